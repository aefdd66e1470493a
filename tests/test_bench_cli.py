"""bench.py's two modes, on the CPU: a plain run is the headline alone (set-up, warm-up, the timed steps, the line),
`--full` adds every sub-run; an option that asks for a sub-run is refused without --full.  run_single is driven with a
recording stand-in for the GPU context at N=32768, the size at which every sub-run of the full line is due."""
import numpy as np
import pytest

import bench
from gp_ss_ak_amd import gpak


def test_plain_run_turns_every_sub_run_off():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full) == (7, 2, False)
    for k, v in bench.PLAIN_VALUES.items():
        assert getattr(a, k) == v, k
    assert not (a.calibrate or a.grad or a.vendor or a.config2 or a.config3 or a.config5)
    assert a.no_cpu and a.no_n65536 and a.grid == "none"


def test_full_run_keeps_the_former_defaults_and_explicit_choices():
    a = bench.parse_args(["--full"])
    for k, v in bench.FULL_DEFAULTS.items():
        assert getattr(a, k) == v, k
    assert not a.no_cpu and not a.no_n65536
    a = bench.parse_args(["--full", "--config2", "0", "--grid", "2x2", "--no-cpu", "--grad", "4"])
    assert (a.config2, a.grid, a.no_cpu, a.grad, a.config5) == (0, "2x2", True, 4, 1000000)


def test_plain_run_accepts_options_that_switch_sub_runs_off():
    a = bench.parse_args(["--no-cpu", "--no-n65536", "--config2", "0", "--config3", "0", "--config5", "0", "--vendor", "0",
                          "--grid", "none", "--grad", "0"])
    assert not a.full and a.config2 == 0 and a.grid == "none"


@pytest.mark.parametrize("opt", [["--grad", "5"], ["--calibrate"], ["--vendor", "1"], ["--config2", "8192"],
                                 ["--config3", "3"], ["--config5", "100"], ["--grid", "2x2"], ["--cpu-n", "4096"]])
def test_plain_run_refuses_an_option_that_asks_for_a_sub_run(opt, capsys):
    with pytest.raises(SystemExit) as e:
        bench.parse_args(opt)
    assert e.value.code == 2 and "--full" in capsys.readouterr().err


def test_dump_outputs_is_refused_off_the_single_context_path(monkeypatch):
    for k in ("WORLD_SIZE", "GPAK_FORCE_DIST"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit):
        bench.parse_args(["--gpus", "2", "--dump-outputs", "d"])
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"


class _FakeCtx:
    """Records what run_single asks of a context; answers with fixed, plausible numbers."""
    calls = []

    def __init__(self, device=0, precision=gpak.F64):
        self.precision, self.N, self.nlz = precision, 0, 0.0
        self.calls.append(("create", precision))

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        self.calls.append((name, None))
        return lambda *a, **k: None

    def set_train(self, X, y):
        self.N = len(y)
        self.calls.append(("set_train", self.N))

    def set_params(self, e, bias, sn2, mode):
        self.nlz = float(-1000.0 * sn2 - e[1] - e[3])         # differs from step to step, like the real one

    def logLikelihood(self):
        self.calls.append(("logLikelihood", self.N))
        return self.nlz

    def timing(self):
        t = dict.fromkeys(("gram_ms", "factor_ms", "solve_ms", "nlz_ms", "kmatvec_ms", "trailing_ms", "trailing_flops",
                           "trailing_bytes", "gram_bytes", "grad_ms"), 1.0)
        t.update(trailing_launches=1, n_padded=self.N)
        return t

    def nlz_terms(self):
        return (1.0, 2.0, self.nlz)

    def solve_alpha(self):
        return np.full(self.N, self.nlz)

    def calibrate(self):
        self.calls.append(("calibrate", None))
        return 70.0, 5000.0

    def GradLL(self):
        self.calls.append(("GradLL", None))
        return np.zeros(10)

    def posteriorMeanVar(self, Xte, want_var=True, compat=0):
        self.calls.append(("posteriorMeanVar", len(Xte)))
        return np.ones(len(Xte)), np.ones(len(Xte))


def _run(monkeypatch, argv):
    _FakeCtx.calls = []
    extras = []
    monkeypatch.setattr(gpak, "Gpak", _FakeCtx)
    monkeypatch.setattr(bench, "cpu_baseline", lambda n, s: extras.append(("cpu_baseline", n, s)) or
                        {"sample_s_per_step": 1.0, "lean_sample_s_per_step": 1.0, "cores": 1, "kind": "port",
                         "sample": "", "nlz_sample": 1.0})
    monkeypatch.setattr(bench, "vendor_potrf", lambda sizes: extras.append(("vendor_potrf", tuple(sizes))) or {})
    monkeypatch.setattr(bench, "config3", lambda iters, n: extras.append(("config3", iters, n)) or {})
    return bench.run_single(bench.parse_args(argv)), _FakeCtx.calls, extras


def test_plain_run_single_is_set_up_warm_up_steps_and_outputs(monkeypatch, tmp_path):
    out, calls, extras = _run(monkeypatch, ["--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path)])
    assert extras == []
    assert [c for c in calls if c[0] in ("create", "set_train", "calibrate", "GradLL", "posteriorMeanVar")] == \
        [("create", gpak.F64), ("set_train", 32768)]
    assert calls.count(("logLikelihood", 32768)) == 5 and len([c for c in calls if c[0] == "logLikelihood"]) == 5
    assert not {"cpu_baseline", "n65536", "config2", "config3", "config5", "vendor_potrf", "grad_step"} & set(out)
    assert "calibrated_mfma_f64_tflops" not in out["roofline"]
    assert out["steps"] == 3 and out["warmup"] == 2 and out["ms_per_step"] > 0
    # the outputs are those of the LAST timed step (index warmup + steps - 1), not of a step run afterwards
    e, _, sn2 = bench.params_for_step(4)
    last = -1000.0 * sn2 - e[1] - e[3]
    assert np.load(tmp_path / "nlz.npy").tolist() == [last] == [out["nlz"]]
    assert np.load(tmp_path / "nlz_terms.npy").tolist() == [1.0, 2.0, last]
    alpha = np.load(tmp_path / "alpha.npy")
    assert alpha.dtype == np.float64 and alpha.shape == (32768,) and np.all(alpha == last)


def test_full_run_single_runs_every_sub_run(monkeypatch):
    out, calls, extras = _run(monkeypatch, ["--steps", "1", "--warmup", "0", "--full", "--grad", "1", "--config5", "1000"])
    assert [x[0] for x in extras] == ["vendor_potrf", "config3", "cpu_baseline", "cpu_baseline"]
    names = {c[0] for c in calls}
    assert {"calibrate", "GradLL", "posteriorMeanVar"} <= names and ("create", gpak.F32) in calls
    assert {("set_train", 65536), ("set_train", 8192)} <= set(calls)
    assert {"cpu_baseline", "n65536", "config2", "config3", "config5", "vendor_potrf", "grad_step"} <= set(out)
    assert "calibrated_mfma_f64_tflops" in out["roofline"]
