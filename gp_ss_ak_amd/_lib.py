"""Loader of libgpak_hip.so (the C-ABI declared in include/gpak.h).

There is no fallback of any kind: if the shared object is missing, cannot be
loaded, or lacks a declared symbol, importing the binding raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPAK_LIB_PATH: tests load a sanitizer build of the same sources (csrc/Makefile targets tsan / asan); never a fallback
LIB_PATH = os.environ.get("GPAK_LIB_PATH") or os.path.join(_HERE, "libgpak_hip.so")

# every symbol include/gpak.h declares (tests check the header and this list agree)
SYMBOLS = [
    "gpak_create", "gpak_create_multi", "gpak_n_gpus", "gpak_transport", "gpak_destroy", "gpak_last_error", "gpak_global_error", "gpak_set_train",
    "gpak_set_params", "gpak_set_kernel", "gpak_set_option", "gpak_gram", "gpak_compute_k", "gpak_factor",
    "gpak_get_chol_upper", "gpak_failed_column", "gpak_solve_alpha", "gpak_solve_chol", "gpak_nlz",
    "gpak_nlz_terms", "gpak_predict", "gpak_grad", "gpak_grad_hyb", "gpak_grad_exact", "gpak_loo", "gpak_block_cross", "gpak_predict_block", "gpak_predict_joint", "gpak_sample_joint", "gpak_timing", "gpak_calibrate", "gpak_reload_tuning",
]
# every symbol include/gpak_loo_grad.h declares (tests/test_loo_grad.py checks the header and this list agree)
LOO_GRAD_SYMBOLS = ["gpak_loo_grad"]
# every symbol include/gpak_cv_groups.h declares (tests/test_cv_groups.py checks the header and this list agree)
CV_GROUPS_SYMBOLS = ["gpak_cv_groups"]
# every symbol include/gpak_cv_folds.h declares (tests/test_cv_folds.py checks the header and this list agree)
CV_FOLDS_SYMBOLS = ["gpak_cv_folds"]
# every symbol include/gpak_cv_groups_grad.h declares (tests/test_cv_groups_grad.py checks the header and this list agree)
CV_GROUPS_GRAD_SYMBOLS = ["gpak_cv_groups_grad"]
# every symbol include/gpak_cv_folds_grad.h declares (tests/test_cv_folds_grad.py checks the header and this list agree)
CV_FOLDS_GRAD_SYMBOLS = ["gpak_cv_folds_grad"]
# every symbol include/gpak_dev_cv_mix.h declares (the same test)
DEV_CV_MIX_SYMBOLS = ["gpak_dev_mix_cols"]
# every symbol include/gpak_dev_cv_kernels.h declares (tests/test_cv_kernels.py checks the header and this list agree)
DEV_CV_KERNELS_SYMBOLS = ["gpak_dev_cvg_gram", "gpak_dev_cvg_solve", "gpak_dev_cvg_mix", "gpak_dev_cvf_pad", "gpak_dev_cvf_w",
                          "gpak_dev_cvf_ev", "gpak_dev_cvf_sums", "gpak_dev_cvf_beta", "gpak_dev_cvf_q", "gpak_dev_cvf_gather",
                          "gpak_dev_cvf_unmix", "gpak_dev_loo_rowsumsq", "gpak_dev_loo_finish", "gpak_dev_loo_vectors",
                          "gpak_dev_loo_mirror_scale", "gpak_dev_loo_rank2", "gpak_dev_lgo_colscale"]
# every symbol include/gpak_design.h / include/gpak_dev_design.h declares (tests/test_design.py checks the headers and these lists agree)
DESIGN_SYMBOLS = ["gpak_design"]
DEV_DESIGN_SYMBOLS = ["gpak_dev_design_score"]
# every symbol include/gpak_condition.h / include/gpak_dev_condition.h declares (tests/test_path.py checks the headers and these lists agree)
CONDITION_SYMBOLS = ["gpak_condition", "gpak_sample_path"]
DEV_CONDITION_SYMBOLS = ["gpak_dev_kmm", "gpak_dev_kmm_slabs", "gpak_dev_kmm_slab_len"]
# every symbol include/gpak_local.h / include/gpak_dev_local.h declares (tests/test_local.py checks the headers and these lists agree)
LOCAL_SYMBOLS = ["gpak_local_metric", "gpak_local_neighbours", "gpak_predict_local"]
DEV_LOCAL_SYMBOLS = ["gpak_dev_local_krige"]
# every symbol include/gpak_local_ok.h / include/gpak_dev_local_ok.h declares (tests/test_local_ok.py checks the headers and these lists agree)
LOCAL_OK_SYMBOLS = ["gpak_predict_local_ok", "gpak_local_neighbours_octant"]
DEV_LOCAL_OK_SYMBOLS = ["gpak_dev_local_krige_ok"]
# every symbol include/gpak_local_search.h / include/gpak_dev_local_search.h declares (tests/test_local_search.py checks the headers and these lists agree)
LOCAL_SEARCH_SYMBOLS = ["gpak_local_neighbours_dev"]
DEV_LOCAL_SEARCH_SYMBOLS = ["gpak_dev_local_search"]
# every symbol include/gpak_dev_f32.h declares (tests/test_dev_ops.py checks the header and this list agree)
DEV_F32_SYMBOLS = ["gpak_dev_gemm_nt_f32", "gpak_dev_fill_f32", "gpak_dev_lower_to_f32", "gpak_dev_vec_to_f32",
                   "gpak_dev_rowsumsq_f32", "gpak_dev_fwd_subst_f32"]


class PhaseTimes(C.Structure):
    _fields_ = [("gram_ms", C.c_double), ("factor_ms", C.c_double), ("solve_ms", C.c_double),
                ("nlz_ms", C.c_double), ("predict_ms", C.c_double), ("grad_ms", C.c_double),
                ("trailing_ms", C.c_double), ("trailing_flops", C.c_double),
                ("trailing_launches", C.c_int), ("gram_bytes", C.c_double), ("n", C.c_int),
                ("n_padded", C.c_int), ("trailing_bytes", C.c_double), ("kmatvec_ms", C.c_double),
                ("accumulated_ms", C.c_double * 4), ("evaluations", C.c_int)]


class LooSummary(C.Structure):
    _fields_ = [("mse", C.c_double), ("mssr", C.c_double), ("log_pl", C.c_double), ("ms", C.c_double),
                ("passes", C.c_int)]


class CvGroupsSummary(C.Structure):
    _fields_ = [("mse", C.c_double), ("mssr", C.c_double), ("msmd", C.c_double), ("log_pl", C.c_double),
                ("ms", C.c_double), ("groups", C.c_int), ("max_size", C.c_int)]


class DesignSummary(C.Structure):
    _fields_ = [("var_before", C.c_double), ("var_after", C.c_double), ("ms", C.c_double), ("holes", C.c_int),
                ("max_size", C.c_int), ("picks", C.c_int)]


class ConditionSummary(C.Structure):
    _fields_ = [("solve_ms", C.c_double), ("prior_ms", C.c_double), ("product_ms", C.c_double), ("batches", C.c_int),
                ("fused", C.c_int)]


class LocalSummary(C.Structure):
    _fields_ = [("upload_ms", C.c_double), ("krige_ms", C.c_double), ("nodes", C.c_long), ("empty", C.c_long),
                ("notpd", C.c_long), ("batches", C.c_int), ("max_used", C.c_int)]


class LocalSearchSummary(C.Structure):
    _fields_ = [("grid_ms", C.c_double), ("upload_ms", C.c_double), ("search_ms", C.c_double), ("centres", C.c_long),
                ("cells", C.c_long), ("visited", C.c_ulonglong), ("batches", C.c_int), ("max_used", C.c_int)]


_lib = None


def load():
    """Returns the ctypes handle; raises RuntimeError if the HIP library is unusable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). gp_ss_ak_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    missing = [s for s in SYMBOLS + LOO_GRAD_SYMBOLS + CV_GROUPS_SYMBOLS + CV_FOLDS_SYMBOLS + CV_GROUPS_GRAD_SYMBOLS
               + CV_FOLDS_GRAD_SYMBOLS + DEV_CV_MIX_SYMBOLS + DESIGN_SYMBOLS + DEV_DESIGN_SYMBOLS + CONDITION_SYMBOLS + DEV_CONDITION_SYMBOLS
               + DEV_F32_SYMBOLS + LOCAL_SYMBOLS + DEV_LOCAL_SYMBOLS + DEV_CV_KERNELS_SYMBOLS
               + LOCAL_OK_SYMBOLS + DEV_LOCAL_OK_SYMBOLS + LOCAL_SEARCH_SYMBOLS + DEV_LOCAL_SEARCH_SYMBOLS
               if not hasattr(lib, s)]
    if missing:
        raise RuntimeError("libgpak_hip.so lacks symbols declared in include/gpak.h / gpak_loo_grad.h / "
                           "gpak_cv_groups.h / gpak_cv_folds.h / gpak_cv_groups_grad.h / gpak_cv_folds_grad.h / "
                           "gpak_dev_cv_mix.h / gpak_design.h / gpak_dev_design.h / gpak_condition.h / gpak_dev_condition.h / "
                           "gpak_dev_f32.h / gpak_local.h / gpak_dev_local.h / gpak_dev_cv_kernels.h / gpak_local_ok.h / "
                           f"gpak_dev_local_ok.h / gpak_local_search.h / gpak_dev_local_search.h: {missing}")
    dp = C.POINTER(C.c_double)
    vp = C.c_void_p
    lib.gpak_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    lib.gpak_create_multi.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int), C.c_int]
    lib.gpak_n_gpus.argtypes = [vp]
    lib.gpak_transport.argtypes = [vp]
    lib.gpak_transport.restype = C.c_char_p
    lib.gpak_destroy.argtypes = [vp]
    lib.gpak_destroy.restype = None
    lib.gpak_last_error.argtypes = [vp]
    lib.gpak_last_error.restype = C.c_char_p
    lib.gpak_global_error.restype = C.c_char_p
    lib.gpak_set_train.argtypes = [vp, dp, dp, C.c_int, C.c_int]
    lib.gpak_set_params.argtypes = [vp, dp, C.c_double, C.c_double, C.c_int]
    lib.gpak_set_kernel.argtypes = [vp, C.c_int, C.POINTER(C.c_int), dp, C.c_double, C.c_double, C.c_double, C.c_int]
    lib.gpak_set_option.argtypes = [vp, C.c_int, C.c_long]
    lib.gpak_gram.argtypes = [vp, dp, dp]
    lib.gpak_compute_k.argtypes = [vp, dp, C.c_int, dp, C.c_int, C.c_int, dp, dp]
    lib.gpak_factor.argtypes = [vp]
    lib.gpak_get_chol_upper.argtypes = [vp, dp]
    lib.gpak_failed_column.argtypes = [vp]
    lib.gpak_solve_alpha.argtypes = [vp, dp]
    lib.gpak_solve_chol.argtypes = [vp, dp, C.c_int]
    lib.gpak_nlz.argtypes = [vp, dp]
    lib.gpak_nlz_terms.argtypes = [vp, dp, dp, dp]
    lib.gpak_predict.argtypes = [vp, dp, C.c_long, C.c_int, dp, dp, C.c_int]
    lib.gpak_grad.argtypes = [vp, dp]
    lib.gpak_grad_hyb.argtypes = [vp, dp, C.c_int]
    lib.gpak_grad_exact.argtypes = [vp, dp, C.c_int]
    lib.gpak_loo.argtypes = [vp, dp, dp, C.POINTER(LooSummary)]
    lib.gpak_loo_grad.argtypes = [vp, dp, C.c_int, C.POINTER(LooSummary)]
    lib.gpak_cv_groups.argtypes = [vp, C.POINTER(C.c_int), C.c_int, dp, dp, dp, C.POINTER(CvGroupsSummary)]
    lib.gpak_cv_folds.argtypes = [vp, C.POINTER(C.c_int), C.c_int, dp, dp, dp, C.POINTER(CvGroupsSummary), C.c_int]
    lib.gpak_cv_groups_grad.argtypes = [vp, C.POINTER(C.c_int), C.c_int, dp, C.c_int, C.POINTER(CvGroupsSummary)]
    lib.gpak_cv_folds_grad.argtypes = [vp, C.POINTER(C.c_int), C.c_int, dp, C.c_int, C.POINTER(CvGroupsSummary), C.c_int]
    # include/gpak_dev_cv_mix.h: the stream first, every pointer a device pointer
    lib.gpak_dev_mix_cols.argtypes = [vp, vp, C.c_long, C.c_int, vp, C.c_int, vp, C.c_long, vp, C.c_long]
    lib.gpak_design.argtypes = [vp, dp, C.c_long, C.c_int, dp, C.c_long, C.c_int, C.POINTER(C.c_int), C.c_int, dp, C.c_int, dp, dp, dp,
                                C.POINTER(C.c_int), dp, dp, C.POINTER(DesignSummary)]
    # include/gpak_dev_design.h: the stream first, every pointer a device pointer
    lib.gpak_dev_design_score.argtypes = [vp, vp, C.c_long, C.c_int, vp, vp, vp, C.c_int, C.c_double, vp, vp, vp, C.c_long, vp]
    ip = C.POINTER(C.c_int)
    lib.gpak_condition.argtypes = [vp, dp, C.c_long, C.c_int, C.c_int, dp, dp, C.c_int, dp, dp, C.c_int, C.POINTER(ConditionSummary)]
    lib.gpak_sample_path.argtypes = [vp, dp, C.c_long, C.c_int, C.c_int, C.c_int, ip, dp, dp, dp, dp, C.c_int, dp, dp, C.c_int,
                                     C.POINTER(ConditionSummary)]
    # include/gpak_dev_condition.h: the stream first, every pointer a device pointer
    lib.gpak_dev_kmm.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, dp, C.c_double, C.c_int, vp, C.c_long,
                                 C.c_int, vp, C.c_long, vp, C.c_long, vp]
    lib.gpak_dev_kmm_slabs.argtypes = [C.c_int]
    lib.gpak_dev_kmm_slab_len.argtypes = [C.c_int]
    lib.gpak_block_cross.argtypes = [vp, dp, C.c_long, C.c_int, C.c_int, dp]
    lib.gpak_predict_block.argtypes = [vp, dp, C.c_long, C.c_int, C.c_int, dp, dp, C.c_int]
    lib.gpak_predict_joint.argtypes = [vp, dp, C.c_long, C.c_int, C.c_int, dp, dp, C.c_int]
    lib.gpak_sample_joint.argtypes = [vp, dp, C.c_long, C.c_int, C.c_int, dp, C.c_int, C.c_double, dp, dp, C.c_int]
    lib.gpak_timing.argtypes = [vp, C.POINTER(PhaseTimes)]
    lib.gpak_calibrate.argtypes = [vp, dp, dp]
    lib.gpak_reload_tuning.restype = None
    # include/gpak_dev_f32.h: the stream first, every pointer a device pointer
    fp, ip = C.c_void_p, C.POINTER(C.c_int)
    lib.gpak_dev_gemm_nt_f32.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_float, fp, C.c_long, fp, C.c_long, C.c_float, fp, C.c_long]
    lib.gpak_dev_fill_f32.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, C.c_double, C.c_int,
                                      fp, C.c_long]
    lib.gpak_dev_lower_to_f32.argtypes = [vp, vp, C.c_long, C.c_int, fp, C.c_long]
    lib.gpak_dev_vec_to_f32.argtypes = [vp, vp, C.c_long, fp]
    lib.gpak_dev_rowsumsq_f32.argtypes = [vp, fp, C.c_long, C.c_int, C.c_int, C.c_int, vp, C.c_int]
    lib.gpak_dev_fwd_subst_f32.argtypes = [vp, fp, C.c_long, C.c_int, C.c_int, fp, C.c_long, fp, ip, C.c_int]
    # include/gpak_local.h; include/gpak_dev_local.h: the stream first, every pointer but kern a device pointer
    lib.gpak_local_metric.argtypes = [vp, C.c_int, dp]
    lib.gpak_local_neighbours.argtypes = [dp, C.c_long, C.c_int, dp, C.c_long, dp, C.c_int, C.c_double, C.c_int, ip, ip]
    lib.gpak_predict_local.argtypes = [vp, dp, dp, C.c_long, C.c_int, dp, C.c_long, C.c_int, ip, C.c_int, dp, dp, C.c_int,
                                       C.POINTER(LocalSummary)]
    lib.gpak_dev_local_krige.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, dp, C.c_double, C.c_int,
                                         C.c_double, C.c_double, vp, C.c_int, C.c_int, vp, vp, vp]
    # include/gpak_local_ok.h; include/gpak_dev_local_ok.h: the stream first, every pointer but kern a device pointer
    lib.gpak_predict_local_ok.argtypes = [vp, dp, dp, C.c_long, C.c_int, dp, C.c_long, C.c_int, ip, C.c_int, dp, dp, dp, C.c_int,
                                          C.POINTER(LocalSummary)]
    lib.gpak_local_neighbours_octant.argtypes = [dp, C.c_long, C.c_int, dp, C.c_long, dp, C.c_int, C.c_int, C.c_double, C.c_int,
                                                 ip, ip]
    lib.gpak_dev_local_krige_ok.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, dp, C.c_double, C.c_int,
                                            C.c_double, C.c_double, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    # include/gpak_local_search.h; include/gpak_dev_local_search.h: the stream first, every pointer a device pointer
    lib.gpak_local_neighbours_dev.argtypes = [vp, dp, C.c_long, C.c_int, dp, C.c_long, dp, C.c_int, C.c_double, ip, ip, dp,
                                              C.POINTER(LocalSearchSummary)]
    lib.gpak_dev_local_search.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                          C.c_int, C.c_int, C.c_int, C.c_double, vp, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp]
    # include/gpak_dev_cv_kernels.h: the stream first, every pointer a device pointer
    i, l, d = C.c_int, C.c_long, C.c_double
    lib.gpak_dev_cvg_gram.argtypes = [vp, vp, l, i, vp, vp, i, vp, vp]
    lib.gpak_dev_cvg_solve.argtypes = [vp, vp, vp, vp, vp, i, i, vp, vp, d, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.gpak_dev_cvg_mix.argtypes = [vp, vp, l, i, vp, vp, i, vp]
    lib.gpak_dev_cvf_pad.argtypes = [vp, vp, l, i]
    lib.gpak_dev_cvf_w.argtypes = [vp, vp, l, i, vp, vp, vp]
    lib.gpak_dev_cvf_ev.argtypes = [vp, vp, l, i, vp, vp, vp, d, vp, vp, vp, vp, vp]
    lib.gpak_dev_cvf_sums.argtypes = [vp, vp, l, i, vp, vp, vp, vp, d, vp, vp, vp]
    lib.gpak_dev_cvf_beta.argtypes = [vp, vp, i, d, vp]
    lib.gpak_dev_cvf_q.argtypes = [vp, i, vp, l, i, vp, vp, vp, vp, vp, l, vp]
    lib.gpak_dev_cvf_gather.argtypes = [vp, vp, l, i, vp, i, vp, l]
    lib.gpak_dev_cvf_unmix.argtypes = [vp, vp, l, i, vp, i, vp, l]
    lib.gpak_dev_loo_rowsumsq.argtypes = [vp, vp, l, i, i, i, vp, vp]
    lib.gpak_dev_loo_finish.argtypes = [vp, i, vp, vp, vp, d, vp, vp, vp, vp]
    lib.gpak_dev_loo_vectors.argtypes = [vp, i, i, vp, vp, d, vp, vp]
    lib.gpak_dev_loo_mirror_scale.argtypes = [vp, i, i, vp, l, vp, vp, l]
    lib.gpak_dev_loo_rank2.argtypes = [vp, i, vp, l, vp, vp]
    lib.gpak_dev_lgo_colscale.argtypes = [vp, i, i, d, vp]
    _lib = lib
    return lib
