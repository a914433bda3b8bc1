"""The Levenberg step the LM kernels share (csrc/orbx_lm.h: lm::trial, lm::iteration_end), host build,
against its Python twin (optsim3_literal.lm_trial / lm_iteration_end) bit for bit.  No GPU.

The twin is what tests/optsim3_literal.py and tests/essgraph_literal.py run; the kernels run the same
header on the device, and the GPU suites hold them to the literals and the oracles.  This test pins the
header's arithmetic where a drift would otherwise show only there: a table with one hand-built state
per branch of OptimizationAlgorithmLevenberg::solve, plus seeded random states, for both cubes
(cube kind 0: x*x*x, the three literal-checked kernels; 1: LocalBundleAdjustment's cube rounded once).

The expected once-rounded cube is the exact rational cube rounded by float(), not math.pow(x, 3): glibc's
pow is within an ulp of it but differs in the last bit on some inputs this test uses (6.118015287389873),
and the library's cube_rounded equals the exact rounding on all of them."""
import collections
import ctypes as C
import math
import struct

import numpy as np
import pytest
import torch  # noqa: F401  (before liborbx.so is loaded, as in the other suites: one HIP runtime per process)

import optsim3_literal as lit

INF, NAN = float("inf"), float("nan")
CUBES = {0: lit.cube_product, 1: lit.cube_rounded}


def bits(*v):
    return struct.pack("<%dd" % len(v), *v)


@pytest.fixture(scope="module")
def step():
    from orb_slam2_commit_amd import _lib
    L = _lib.lib()

    def run(state, iniChi, tempChi, scale, ok2, kind, ops):
        """state as the twin's (lam, ni, currentChi, rho, qmax, nBad) -> (state, flags)"""
        lam, ni, cur, rho, qmax, nBad = state
        d = (C.c_double * 5)(lam, ni, cur, iniChi, rho)
        k = (C.c_int * 2)(qmax, nBad)
        r = L.orbx_debug_lm_step(d, k, tempChi, scale, int(ok2), kind, ops)
        assert r >= 0 and bits(d[3]) == bits(iniChi)
        return (d[0], d[1], d[2], d[4], k[0], k[1]), r
    return run


def same(a, b):
    return bits(*a[:4]) == bits(*b[:4]) and tuple(a[4:]) == tuple(b[4:])


def check(step, row, kind, counters):
    """One row through the trial verdict and, when no further trial follows, the iteration-end rule."""
    state, iniChi, tempChi, scale, ok2 = row
    exp, accept, go = lit.lm_trial(state, tempChi, scale, ok2, cube=CUBES[kind], counters=counters)
    got, r = step(state, iniChi, tempChi, scale, ok2, kind, 1)
    assert same(got, exp) and bool(r & 1) == accept and bool(r & 2) == go and not r & 4, (row, kind, got, exp, r)
    if go:
        return
    exp2, stop = lit.lm_iteration_end(exp, iniChi, counters=counters)
    got2, r2 = step(got, iniChi, 0.0, 0.0, 1, kind, 2)
    assert same(got2, exp2) and bool(r2 & 4) == stop and not r2 & 3, (row, kind, got2, exp2, r2)
    # and both in one call
    got3, r3 = step(state, iniChi, tempChi, scale, ok2, kind, 3)
    assert same(got3, exp2) and r3 == (r | (4 if stop else 0)), (row, kind)


# (lam, ni, currentChi, rho, qmax, nBad), iniChi, tempChi, scale, ok2 -> the branches the row must take
TABLE = [
    # rho ~ 0.4998: alpha ~ 1, clipped at 2/3; a gain of a tenth of iniChi resets nBad
    (((1e-3, 4.0, 10.0, 0.0, 0, 2), 10.0, 9.0, 2.0, True), ("alpha_above_2/3", "nbad_reset")),
    # rho ~ 8.99: alpha < 0, raised to 1/3
    (((1e-3, 2.0, 10.0, 0.0, 0, 0), 10.0, 1.0, 1.0, True), ("alpha_below_1/3", "nbad_reset")),
    # rho = 0.9: alpha = 1 - 0.8^3 = 0.488, used as it is
    (((1e-3, 2.0, 10.0, 0.0, 3, 0), 10.0, 1.0, 9.999, True), ("alpha_between",)),
    # chi rose: rho < 0, reject, another trial
    (((1e-3, 2.0, 10.0, 0.0, 0, 0), 10.0, 12.0, 2.0, True), ("reject_rho_le_0",)),
    # tempChi = -inf: rho = +inf > 0 but the chi is not finite; +inf: rho = -inf
    (((1e-3, 2.0, 10.0, 0.0, 0, 0), 10.0, -INF, 2.0, True), ("reject_nonfinite_chi",)),
    (((1e-3, 8.0, 10.0, 0.0, 2, 0), 10.0, INF, 2.0, True), ("reject_rho_le_0",)),
    # the solve failed: tempChi = DBL_MAX whatever the caller passes
    (((1e-3, 2.0, 10.0, 0.0, 0, 0), 10.0, 5.0, 7.0, False), ("not_ok2", "reject_rho_le_0")),
    # rho NaN (a NaN chi): reject, no further trial, the iteration-end rule counts it
    (((1e-3, 2.0, 10.0, 0.0, 1, 0), 10.0, NAN, 2.0, True), ("reject_rho_nan", "nbad_up")),
    (((1e-3, 2.0, NAN, 0.0, 1, 0), NAN, 3.0, 2.0, True), ("reject_rho_nan", "nbad_reset")),
    # rho == 0: reject and stop
    (((1e-3, 2.0, 10.0, 0.5, 0, 0), 10.0, 10.0, 2.0, True), ("stop_rho_0",)),
    # the tenth trial rejected: stop
    (((1e-3, 1024.0, 10.0, -1.0, 9, 0), 10.0, 12.0, 2.0, True), ("tenth_trial", "stop_qmax_10")),
    # the tenth trial accepted stops all the same
    (((1e-3, 1024.0, 10.0, -1.0, 9, 1), 10.0, 9.0, 2.0, True), ("stop_qmax_10",)),
    # a gain below a thousandth, the third in a row: nBad reaches 3
    (((1e-3, 2.0, 10.0, 0.0, 0, 2), 10.0, 9.9999, 1e-4, True), ("nbad_up", "stop_nbad_3")),
    # the same gain with nBad = 0 goes on
    (((1e-3, 2.0, 10.0, 0.0, 0, 0), 10.0, 9.9999, 1e-4, True), ("nbad_up",)),
]
BRANCHES = ("alpha_above_2/3", "alpha_below_1/3", "alpha_between", "reject_rho_le_0", "reject_nonfinite_chi",
            "reject_rho_nan", "not_ok2", "tenth_trial", "stop_qmax_10", "stop_rho_0", "nbad_up", "nbad_reset",
            "stop_nbad_3")


def random_rows(n, seed):
    """States around a target gain ratio: 40 % inside the band where alpha is used unclipped (there the
    cube's last bit reaches lambda), the rest over rejections, both clips, failed solves and every qmax."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        cur = float(np.exp(rng.uniform(-5, 12)))
        rho_t = float(rng.uniform(0.8467, 0.9368) if rng.random() < 0.4 else rng.uniform(-2.0, 4.0))
        scale = float(np.exp(rng.uniform(-8, 6)))
        temp = cur - rho_t * (scale + 1e-3)
        ini = cur if rng.random() < 0.5 else cur * float(1 + np.exp(rng.uniform(-12, 0)))
        state = (float(np.exp(rng.uniform(-30, 10))), float(2 ** int(rng.integers(1, 11))), cur,
                 float(rng.uniform(-1, 1)), int(rng.integers(0, 10)), int(rng.integers(0, 3)))
        rows.append((state, ini, temp, scale, bool(rng.random() >= 0.05)))
    return rows


@pytest.mark.parametrize("kind", (0, 1))
def test_host_step_equals_the_twin(step, kind):
    counters = collections.Counter()
    for row, want in TABLE:
        c = collections.Counter()
        check(step, row, kind, c)
        assert all(c[b] == 1 for b in want), (row, want, dict(c))
        counters.update(c)
    missing = [b for b in BRANCHES if not counters[b]]
    assert not missing, missing  # the table alone reaches every branch
    for row in random_rows(4000, 20 + kind):
        check(step, row, kind, counters)
    assert counters["alpha_between"] > 1000 and counters["reject_rho_le_0"] > 500 and counters["not_ok2"] > 100


def test_the_two_cubes_differ():
    """The reason the cube is a choice: x*x*x rounds twice, std::pow(x, 3) once, and the kernels follow
    their yardsticks to the bit.  On the band of unclipped alpha the two differ for a good share of x;
    std::pow stays within an ulp of the once-rounded cube."""
    rng = np.random.default_rng(7)
    x = (2 * rng.uniform(0.8467, 0.9368, 2000) - 1).tolist()
    differ = sum(lit.cube_product(v) != lit.cube_rounded(v) for v in x)
    assert differ > 200, differ
    assert all(abs(math.pow(v, 3) - lit.cube_rounded(v)) <= math.ulp(lit.cube_rounded(v)) for v in x)


def test_step_argument_checks(step):
    from orb_slam2_commit_amd import _lib
    L = _lib.lib()
    d, k = (C.c_double * 5)(1, 2, 3, 3, 0), (C.c_int * 2)(0, 0)
    assert L.orbx_debug_lm_step(None, k, 1.0, 1.0, 1, 0, 1) == -1
    assert L.orbx_debug_lm_step(d, None, 1.0, 1.0, 1, 0, 1) == -1
    assert L.orbx_debug_lm_step(d, k, 1.0, 1.0, 1, 2, 1) == -1
    assert L.orbx_debug_lm_step(d, k, 1.0, 1.0, 1, 0, 0) == -1
    assert L.orbx_debug_lm_step(d, k, 1.0, 1.0, 1, 0, 4) == -1
    assert bits(*d) == bits(1, 2, 3, 3, 0) and tuple(k) == (0, 0)
