"""Optimizer::OptimizeSim3 (src/Optimizer.cc:1220-1456), the refinement stage of LoopClosing::ComputeSim3.

CPU: the literal restatement (tests/optsim3_literal.py) checked piece by piece -- its n-unknown
Eigen-LDLT against the oracle's ldlt6 bit for bit, exp_det against its derived error bound, the numeric
Jacobian against the closed form of both edges, convergence / outlier rejection, the early returns, and
the branch counters of the case table.  GPU (-m gpu): the HIP kernel (one block per problem, the whole
schedule on the device) against the literal BIT FOR BIT -- the Sim3 as double bits, the inlier bytes, the
return value, nBad, both iteration counts and the trial count -- on single problems and a device batch,
plus the two debug probes (Sim3's exp branches, exp_det).
Parity vs the genuine g2o/Eigen binary is unpinned, as for PoseOptimization.
"""
import collections
import ctypes as C
import decimal
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle  # noqa: E402
import optsim3_literal as lit  # noqa: E402
import optsim3_scenes as scenes  # noqa: E402
import sim3_scenes  # noqa: E402


# ------------------------------------------------------------------ CPU: the literal's pieces
def _ldlt_inputs():
    rng = np.random.default_rng(0)
    out = []
    for _ in range(25):
        A = rng.normal(0, 1, (6, 6))
        out.append((A @ A.T + 0.1 * np.eye(6), rng.normal(0, 1, 6)))
    for _ in range(25):
        A = rng.normal(0, 1, (6, 6))
        H = A @ A.T + 0.1 * np.eye(6)
        H[np.arange(6), np.arange(6)] *= rng.uniform(0.1, 1e4, 6)  # forces diagonal pivoting
        out.append((H, rng.normal(0, 1, 6)))
    out.append((-np.eye(6) + 0.01 * np.ones((6, 6)), np.ones(6)))  # indefinite: !isPositive()
    out.append((np.zeros((6, 6)), np.ones(6)))                      # ZeroSign
    return out


def test_ldlt_n6_matches_the_oracle_bit_for_bit():
    """ldlt_solve(., ., 6) is oracle/poseopt.cpp's ldlt6: same verdict, same solution bits."""
    oks = []
    for H, b in _ldlt_inputs():
        ok_o, x_o = oracle.ldlt6(H, b)
        ok_l, x_l = lit.ldlt_solve(H.reshape(36).tolist(), b.tolist(), 6)
        assert ok_l == ok_o
        oks.append(ok_o)
        if ok_o:
            assert np.array_equal(np.array(x_l).view(np.uint64), x_o.view(np.uint64))
    assert oks[-2] is False and oks[-1] is True and all(oks[:50])


def test_ldlt_n7_solves():
    rng = np.random.default_rng(1)
    for _ in range(20):
        A = rng.normal(0, 1, (7, 7))
        H = A @ A.T + 0.1 * np.eye(7)
        H[np.arange(7), np.arange(7)] *= rng.uniform(0.1, 1e4, 7)
        b = rng.normal(0, 1, 7)
        ok, x = lit.ldlt_solve(H.reshape(49).tolist(), b.tolist(), 7)
        assert ok and np.allclose(x, np.linalg.solve(H, b), rtol=1e-8, atol=1e-10)


def _exp_grid():
    rng = np.random.default_rng(2)
    return np.concatenate([np.linspace(-2, 2, 4001), rng.uniform(-2, 2, 4000), rng.uniform(-1e-4, 1e-4, 500),
                           (np.arange(-3, 4) * math.log(2) / 2), [0.0, -0.0, 1e-300, 2.0, -2.0]])


def test_exp_det_bound():
    """exp_det is within its derived bound (2.5 * 2^-53 relative, see its docstring) of the true
    exponential on [-2, 2] -- the truth taken from a 50-digit decimal exp -- hence within that plus
    libm's own 1 ulp (2^-52) of math.exp; and exp_det(0) is exactly 1.0 (with bFixScale the update's
    sigma is 0 and s must stay bit-identical under s * 1.0)."""
    assert lit.exp_det(0.0) == 1.0 and lit.exp_det(-0.0) == 1.0
    ctx = decimal.Context(prec=50)
    worst = 0.0
    for x in _exp_grid():
        x = float(x)
        y = lit.exp_det(x)
        true = ctx.exp(decimal.Decimal(x))
        rel = abs(float((decimal.Decimal(y) - true) / true))
        worst = max(worst, rel)
        assert rel <= lit.EXP_DET_BOUND, (x, rel)
        assert abs(y - math.exp(x)) <= (lit.EXP_DET_BOUND + 2.0 ** -52) * math.exp(x), x
    print("exp_det worst relative error / 2^-53: %.3f" % (worst * 2.0 ** 53))


def _closed_form(S, X, K, inverse):
    """d error / d update of EdgeSim3ProjectXYZ (inverse = False) / EdgeInverseSim3ProjectXYZ for the
    left update Sim3(u) * S, u = (omega, upsilon, sigma), by the chain rule in numpy."""
    q, t, s = S
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    t = np.array(t)

    def gen(p):  # d (Sim3(u) p) / du at 0
        px = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        return np.hstack([-px, np.eye(3), p.reshape(3, 1)])
    if not inverse:
        p = s * R @ X + t
        dp = gen(p)
    else:
        p = R.T @ (X - t) / s
        dp = -(R.T / s) @ gen(X)
    fx, fy = K[0], K[1]
    Jp = np.array([[fx / p[2], 0, -fx * p[0] / p[2] ** 2], [0, fy / p[2], -fy * p[1] / p[2] ** 2]])
    return -Jp @ dp


def _jacobian_deviation():
    """Worst |numeric - closed form| / max|closed form| over 20 seeded states, both edges."""
    rng = np.random.RandomState(11)
    worst = 0.0
    for _ in range(20):
        R = sim3_scenes.rotation(rng.normal(size=3), rng.uniform(0.05, 1.0))
        S = lit.sim3_from8(lit.sim3_from_rts(R, rng.normal(0, 0.5, 3), rng.uniform(0.7, 1.5)))
        X = np.array([rng.uniform(-2.5, 2.5), rng.uniform(-1.8, 1.8), rng.uniform(3, 9)])
        for inverse, K in ((False, sim3_scenes.K1), (True, sim3_scenes.K2)):
            Xs = np.array(lit.sim3_map(lit.sim3_inverse(S), list(X))) if not inverse else \
                np.array(lit.sim3_map(S, list(X)))  # a point that lands in front of the camera
            obs = (300.0, 200.0)
            err = lit.error21 if inverse else lit.error12
            J0, J1 = lit.numeric_jacobian(S, False, lambda T: err(T, list(Xs), obs, K))
            Jn = np.array([J0, J1])
            Jc = _closed_form(S, Xs, K, inverse)
            worst = max(worst, np.abs(Jn - Jc).max() / np.abs(Jc).max())
    return worst


def test_numeric_jacobian_against_the_closed_form():
    """The literal's central differences (delta = 1e-9) against the closed-form Jacobian of both edges at
    20 random states.  The worst relative deviation measured on these seeded states is 1.428e-7 of the
    edge's largest entry: difference noise of order ulp(pixel) / delta (~6e-14 / 2e-9 = 3e-5 against
    entries of ~1e2..1e3), not a design number; the assertion is twice that."""
    worst = _jacobian_deviation()
    print("numeric Jacobian worst relative deviation: %.3e" % worst)
    assert worst <= 2 * 1.428e-7


@pytest.mark.parametrize("fix", [0, 1])
def test_literal_recovers_the_truth_and_flags_outliers(fix):
    P = scenes.make_problem(120, 0.25, fix, 77 + fix, pixel_noise=0.0)
    r = lit.optimize_sim3(P)
    s, R, t = P["truth"]
    truth = lit.sim3_from_rts(R, t, s)
    start_err = np.abs(np.asarray(P["S12"]) - truth).max()
    end_err = np.abs(r["S12"] - truth).max()
    assert end_err < 1e-3 and end_err < 0.05 * start_err, (start_err, end_err)
    g = scenes.gross(P)
    assert g.sum() == 30 and (r["inlier"][g] == 0).all() and (r["inlier"][~g] == 1).all()
    assert r["n_in"] == 90 and r["n_bad"] == 30 and r["counters"]["nMore_10"] == 1
    if fix:
        assert r["S12"][7] == P["S12"][7] == 1.0  # s * exp_det(0) stays bit-identical


def test_literal_early_paths():
    P, r = scenes.case("n0")
    assert r["n_in"] == 0 and r["trials"] == 0 and r["iterations"] == [0, 0] and r["counters"]["early_return"] == 1
    assert np.array_equal(r["S12"].view(np.uint64), np.asarray(P["S12"]).view(np.uint64))
    for name in ("n9_early", "n14_early_partial", "n40_out80_early"):
        P, r = scenes.case(name)
        assert r["n_in"] == 0 and r["iterations"][0] > 0 and r["iterations"][1] == 0
        assert r["counters"]["early_return"] == 1 and len(P["x3dc1"]) - r["n_bad"] < 10
        assert np.array_equal(r["S12"].view(np.uint64), np.asarray(P["S12"]).view(np.uint64))  # not written back
        assert int((r["inlier"] == 0).sum()) == r["n_bad"]  # the nulled matches stay nulled
    assert 0 < scenes.case("n14_early_partial")[1]["n_bad"] < 14


def test_case_table_reaches_every_branch():
    """The counters of the literal over the GPU case table: every Sim3 exp branch in an LM step, a
    rejected trial, the stale-error outlier pass, both values of nMore and the early return."""
    total = {}
    for name in scenes.CASES:
        for k, v in scenes.case(name)[1]["counters"].items():
            total[k] = total.get(k, 0) + v
    for b in lit.BRANCHES:
        assert total.get("exp_" + b, 0) > 0, b
    for k in ("rejected_trials", "stale_error_pass", "nMore_5", "nMore_10", "early_return"):
        assert total.get(k, 0) > 0, k
    for name in scenes.FAR:
        assert scenes.case(name)[1]["counters"]["rejected_trials"] > 0, name
    for name in scenes.STALE:
        assert scenes.case(name)[1]["counters"]["stale_error_pass"] == 1, name
    for name in scenes.EARLY:
        assert scenes.case(name)[1]["counters"]["early_return"] == 1, name
    assert {len(scenes.case(n)[0]["x3dc1"]) for n in scenes.CASES} >= {0, 9, 10, 11, 32, 33, 64, 65, 128, 129, 300}


# ------------------------------------------------------------------ GPU
def _same(g, o, n):
    n_in, S12, inlier, n_bad, its, trials = g
    assert n_in == o["n_in"], (n_in, o["n_in"])
    assert n_bad == o["n_bad"], (n_bad, o["n_bad"])
    assert list(its) == list(o["iterations"]), (its, o["iterations"])
    assert trials == o["trials"], (trials, o["trials"])
    assert np.array_equal(np.asarray(inlier)[:n], o["inlier"])
    assert np.array_equal(np.asarray(S12, np.float64).view(np.uint64), o["S12"].view(np.uint64)), (S12, o["S12"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(scenes.CASES))
def test_gpu_optimize_sim3_bit_exact(gpu, name):
    from orb_slam2_commit_amd import Optimizer
    P, o = scenes.case(name)
    opt = Optimizer()
    _same(opt.OptimizeSim3(P), o, len(P["x3dc1"]))
    opt.close()


@pytest.mark.gpu
def test_gpu_optimize_sim3_device_batch(gpu):
    """24 mixed problems through one orbx_optimize_sim3_device launch, each against its own literal run."""
    import torch
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd.orb import optimize_sim3_problem_struct

    probs, keep, refs = [], [], []
    for P in scenes.batch_problems():
        refs.append(lit.optimize_sim3(P))
        n = len(P["x3dc1"])
        d = dict(P)
        for k in ("x3dc1", "x3dc2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
            d[k] = torch.from_numpy(np.ascontiguousarray(P[k], np.float32)).to(gpu)
        outs = dict(S12_out=torch.zeros(8, dtype=torch.float64, device=gpu),
                    inlier=torch.zeros(max(n, 1), dtype=torch.uint8, device=gpu),
                    n_in=torch.zeros(1, dtype=torch.int32, device=gpu),
                    n_bad=torch.zeros(1, dtype=torch.int32, device=gpu),
                    iterations=torch.zeros(2, dtype=torch.int32, device=gpu),
                    trials=torch.zeros(1, dtype=torch.int32, device=gpu))
        p, _ = optimize_sim3_problem_struct(d, outs)
        probs.append(p)
        keep.append((d, outs, n))
    arr = (_lib.OptSim3Problem * len(probs))(*probs)
    s = torch.cuda.current_stream()
    _lib.check(_lib.lib().orbx_optimize_sim3_device(arr, len(probs), C.c_void_p(s.cuda_stream)), "batch")
    torch.cuda.synchronize()
    assert {r["counters"].get("early_return", 0) for r in refs} == {0, 1}
    for (d, outs, n), o in zip(keep, refs):
        g = (int(outs["n_in"].cpu()[0]), outs["S12_out"].cpu().numpy(), outs["inlier"].cpu().numpy(),
             int(outs["n_bad"].cpu()[0]), outs["iterations"].cpu().numpy(), int(outs["trials"].cpu()[0]))
        _same(g, o, n)


PROBE_UPDATES = [  # one per Sim3 exp branch, + the exact zero and a large rotation
    [1e-6, -2e-6, 3e-6, 0.01, -0.02, 0.03, 2e-6],
    [0.1, -0.2, 0.05, 0.01, -0.02, 0.03, -3e-6],
    [1e-6, -2e-6, 3e-6, 0.01, -0.02, 0.03, 0.05],
    [0.1, -0.2, 0.05, 0.01, -0.02, 0.03, -0.07],
    [0.0] * 7,
    [2.0, 1.5, -1.0, 0.3, 0.2, -0.1, 0.4],
    [1e-9, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, -1e-9],
]


@pytest.mark.gpu
def test_gpu_sim3_exp_probe_covers_every_branch(gpu):
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd._lib import ptr
    S = lit.sim3_from_rts(sim3_scenes.rotation([0.3, -1.0, 0.5], 0.7), [0.4, -0.2, 0.3], 1.3)
    seen = collections.Counter()
    for u in PROBE_UPDATES:
        for fix in (0, 1):
            want = lit.sim3_to8(lit.oplus(lit.sim3_from8(S), list(u), fix, seen))
            out = np.zeros(8)
            ua = np.array(u, np.float64)
            _lib.check(_lib.lib().orbx_debug_sim3_exp(ptr(ua), ptr(S), fix, ptr(out), 0), "orbx_debug_sim3_exp")
            assert np.array_equal(out.view(np.uint64), want.view(np.uint64)), (u, fix, out, want)
            if fix:
                assert out[7] == S[7]
    assert all(seen["exp_" + b] > 0 for b in lit.BRANCHES)


@pytest.mark.gpu
def test_gpu_exp_det_grid(gpu):
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd._lib import ptr
    x = np.ascontiguousarray(np.concatenate([_exp_grid(), np.linspace(-700, 700, 1401)]))
    y = np.zeros_like(x)
    _lib.check(_lib.lib().orbx_debug_exp(ptr(x), len(x), ptr(y), 0), "orbx_debug_exp")
    want = np.array([lit.exp_det(v) for v in x])
    assert np.array_equal(y.view(np.uint64), want.view(np.uint64))
