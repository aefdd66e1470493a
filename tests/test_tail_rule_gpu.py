"""-m gpu: the CU-masked tail queue by matrix size (GPAK_TAIL_MAX_NP, gpak_potrf_caps in csrc/potrf_plan.h).  Whether the
tail's bulk updates run on the masked queue or stay on the bulk queue -- and with them which of the two builds of the
block kernel the tail's panels take -- changes where and when a tile is computed, never how: nlZ, its terms and alpha
(and the factor at the two small sizes) must be the same BYTES with no limit (0), with the default, and with a limit
of 1 (the queue is never used), at N = 2048, 8192 and 32768."""
import os

import numpy as np
import pytest

from gp_ss_ak_amd import gpak, synth

pytestmark = pytest.mark.gpu

E = np.array(synth.DEFAULT_EXPANS)
BIAS, SN2 = synth.DEFAULT_BIAS, synth.DEFAULT_SN2
KEYS = ("GPAK_TAIL_MAX_NP", "GPAK_TAIL_ROWS", "GPAK_TAIL_MASK", "GPAK_BULK_QUEUE", "GPAK_POTRF_CO")


def run(X, y, env, want_factor):
    """nlZ, its three terms, alpha and (want_factor) the factor of one fresh context made under `env`."""
    from gp_ss_ak_amd import _lib
    lib = _lib.load()
    saved = {k: os.environ.get(k) for k in KEYS}
    try:
        for k in KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        lib.gpak_reload_tuning()
        g = gpak.Gpak(0)
        try:
            g.set_train(X, y)
            g.set_params(E, BIAS, SN2, gpak.DIST_DIRECT)
            out = [np.array([g.logLikelihood()]), np.array(g.nlz_terms(), dtype=np.float64), g.solve_alpha()]
            if want_factor:
                out.append(g.chol_upper())
        finally:
            g.close()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.gpak_reload_tuning()
    return out


def same_bytes(a, b):
    return all(x.dtype == z.dtype and x.shape == z.shape and x.tobytes() == z.tobytes() for x, z in zip(a, b))


@pytest.mark.parametrize("N", [2048, 8192, 32768])
def test_tail_queue_limit_same_bytes(N):
    X, y = synth.drillholes(N)
    want = N <= 8192
    ref = run(X, y, {"GPAK_TAIL_MAX_NP": "0"}, want)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[2]).all()
    assert same_bytes(run(X, y, {}, want), ref), "default"
    assert same_bytes(run(X, y, {"GPAK_TAIL_MAX_NP": "1"}, want), ref), "queue never used"


def test_option_sets_the_limit():
    """The same through gpak_set_option on one context: the option is read at the next factorisation."""
    X, y = synth.drillholes(2048)
    g = gpak.Gpak(0)
    try:
        g.set_train(X, y)
        got = []
        for limit in (0, 1, 1024, 4096):
            g.set_option(gpak.OPT_TAIL_MAX_NP, limit)
            g.set_params(E, BIAS, SN2, gpak.DIST_DIRECT)
            got.append([np.array([g.logLikelihood()]), g.solve_alpha()])
        with pytest.raises(gpak.GpakError):
            g.set_option(gpak.OPT_TAIL_MAX_NP, -1)
    finally:
        g.close()
    assert all(same_bytes(x, got[0]) for x in got[1:])
