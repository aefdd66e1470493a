"""-m gpu: the ticketed tile map of the factorisation's bulk update (GPAK_BULK_TICKETS=1, gemm.hip TICKET) against the
static blockIdx map (GPAK_BULK_TICKETS=0).  Only the choice of which workgroup computes which tile differs, so the
factor, alpha and nlZ must be the same BYTES: on the CU-masked tail queue and on the plain queue, with no surplus
workgroups and with many, at tile counts that are and are not multiples of an XCD's 64 slots, and in full
factorisations at N = 2048, 8192 and 32768."""
import os

import numpy as np
import pytest

from gp_ss_ak_amd import gpak, synth

pytestmark = pytest.mark.gpu

E = np.array(synth.DEFAULT_EXPANS)
BIAS, SN2 = synth.DEFAULT_BIAS, synth.DEFAULT_SN2
KEYS = ("GPAK_BULK_TICKETS", "GPAK_BULK_SURPLUS", "GPAK_TAIL_ROWS", "GPAK_TAIL_MASK", "GPAK_BULK_QUEUE",
        "GPAK_NB_OUTER", "GPAK_NB_WIDE", "GPAK_NB_XWIDE")


def run(X, y, env, want_factor):
    """nlZ, its three terms, alpha and (want_factor) the factor of one context made under `env`."""
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


CASES = [
    {},
    {"GPAK_TAIL_ROWS": "100000"},                                  # every bulk update on the CU-masked tail queue
    {"GPAK_TAIL_MASK": "0", "GPAK_BULK_QUEUE": "0"},               # every bulk update on the context's plain stream
    {"GPAK_BULK_SURPLUS": "0"},                                    # exactly one workgroup per tile
    {"GPAK_BULK_SURPLUS": "100", "GPAK_TAIL_ROWS": "100000"},      # twice as many workgroups as tiles
    {"GPAK_NB_OUTER": "384", "GPAK_NB_WIDE": "0", "GPAK_NB_XWIDE": "0"},
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_tickets_equal_static_map_bytes(case):
    """N = 5000 (a partial last tile): every knob combination, factor included."""
    X, y = synth.drillholes(5000)
    env = CASES[case]
    ref = run(X, y, dict(env, GPAK_BULK_TICKETS="0"), True)
    got = run(X, y, dict(env, GPAK_BULK_TICKETS="1"), True)
    assert same_bytes(got, ref), env


def test_tickets_tile_counts_multiple_of_xcd_slots():
    """128-column panels over 130 tile rows: one bulk update for every trailing size from 128 tile rows down, among them
    8256 = 129 x 64 and 8128 = 127 x 64 tiles (whole rounds of an XCD's 64 slots) and all the counts in between."""
    X, y = synth.drillholes(130 * 128)
    env = {"GPAK_NB_OUTER": "128", "GPAK_NB_WIDE": "0", "GPAK_NB_XWIDE": "0", "GPAK_BULK_SURPLUS": "0"}
    ref = run(X, y, dict(env, GPAK_BULK_TICKETS="0"), False)
    got = run(X, y, dict(env, GPAK_BULK_TICKETS="1"), False)
    assert same_bytes(got, ref)


@pytest.mark.parametrize("N", [2048, 8192, 32768])
def test_tickets_full_factorisation_bytes(N):
    """The default schedule at the bench's sizes: nlZ, its terms and alpha (and the factor up to N = 8192)."""
    X, y = synth.drillholes(N)
    want = N <= 8192
    ref = run(X, y, {"GPAK_BULK_TICKETS": "0"}, want)
    got = run(X, y, {"GPAK_BULK_TICKETS": "1"}, want)
    assert same_bytes(got, ref)
