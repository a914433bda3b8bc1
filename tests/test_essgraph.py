"""Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:888-1218), the pose graph of LoopClosing::CorrectLoop.

CPU: the literal restatement (tests/essgraph_literal.py) checked piece by piece -- log_det / acos_det against
their derived bounds, Sim3's log against its exp, the numeric Jacobians against a closed form, the LDL^T
solve against numpy, convergence on the ring scenes, the branch counters of the scene set, and the Python
mirror's edge selection against a hand-listed edge set.  GPU (-m gpu): the HIP kernels against the literal
BIT FOR BIT -- the probes (log_det, acos_det, sim3_log, the first linearisation, one solve) and the whole
run on every scene (Sim3s as double bits, poses and points as float bits, iteration and trial counts, both
chi2), host form and stream form.
Parity vs the genuine g2o/Eigen binary is unpinned, as for PoseOptimization and OptimizeSim3.
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import essgraph_literal as lit  # noqa: E402
import essgraph_scenes as scenes  # noqa: E402
import optsim3_literal as osl  # noqa: E402
import sim3_literal  # noqa: E402

U = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------ CPU: the twins
def _log_grid():
    rng = np.random.default_rng(3)
    return np.concatenate([rng.uniform(0.5, 2.0, 3000), 1 + rng.uniform(-1e-4, 1e-4, 500), 1 + rng.uniform(-1e-9, 1e-9, 200),
                           np.exp(rng.uniform(-700, 700, 1500)), 2.0 ** np.arange(-20, 21),
                           np.sqrt(2.0) * (1 + np.arange(-4, 5) * 2.0 ** -52), [1.0, 0.7, 1.3, 2.2250738585072014e-308,
                                                                                1.7976931348623157e308]])


def _acos_grid():
    rng = np.random.default_rng(4)
    return np.concatenate([rng.uniform(-1, 1, 3000), 1 - 10.0 ** rng.uniform(-15, -1, 1000),
                           -1 + 10.0 ** rng.uniform(-15, -1, 300), np.arange(-8, 9) / 8.0,
                           [1 - 0.00001, 1 - 0.00001 - 2.0 ** -50, 0.0, -0.0, 1.0, -1.0]])


def test_log_det_bound():
    """log_det is within its derived bound (6 * 2^-53 relative, see its docstring) of the true logarithm,
    taken from a 50-digit decimal ln; log_det(1.0) is exactly 0.0 (a scale of 1 must give sigma == 0 and the
    |sigma| < eps branch)."""
    assert lit.log_det(1.0) == 0.0 and not math.copysign(1.0, lit.log_det(1.0)) < 0
    assert math.isnan(lit.log_det(0.0)) and math.isnan(lit.log_det(-1.0)) and math.isnan(lit.log_det(float("inf")))
    ctx = decimal.Context(prec=50)
    x = _log_grid()
    y = lit.log_det(x)
    worst = 0.0
    for a, b in zip(x.tolist(), y.tolist()):
        true = ctx.ln(decimal.Decimal(a))
        if true == 0:
            assert b == 0.0
            continue
        rel = abs(float((decimal.Decimal(b) - true) / true))
        worst = max(worst, rel)
        assert rel <= lit.LOG_DET_BOUND, (a, rel / U)
        assert lit.log_det(a) == b  # the scalar path is the array path
    print("log_det worst relative error / 2^-53: %.3f" % (worst / U))


def _acos_true(x, ctx):
    """acos x = 2 atan(sqrt((1 - x) / (1 + x))) to ~45 digits (decimal has no atan: halve the argument
    three times with atan t = 2 atan(t / (1 + sqrt(1 + t^2))), then the odd series)."""
    D = decimal.Decimal
    x = D(x)
    if x == -1:
        return None
    t = ctx.sqrt(ctx.divide(ctx.subtract(D(1), x), ctx.add(D(1), x)))
    halvings = 0
    while t > D("0.05"):
        t = ctx.divide(t, ctx.add(D(1), ctx.sqrt(ctx.add(D(1), ctx.multiply(t, t)))))
        halvings += 1
    t2 = ctx.multiply(t, t)
    term, s, k = t, t, 1
    while abs(term) > D(10) ** -48:
        term = -ctx.multiply(term, t2)
        k += 2
        s = ctx.add(s, ctx.divide(term, D(k)))
    return ctx.multiply(s, D(2 ** (halvings + 1)))


def test_acos_det_bound():
    """acos_det is within its derived bound (20 * 2^-53 relative, see its docstring) of the true arc cosine
    on [-1, 1), the truth from 50-digit decimal arithmetic; acos_det(1) is exactly 0 and the array twins of
    atan2_det / sincos_d equal tests/sim3_literal.py's scalar ones bit for bit."""
    assert lit.acos_det(1.0) == 0.0 and math.isnan(lit.acos_det(1.0000001))
    ctx = decimal.Context(prec=50)
    x = _acos_grid()
    y = lit.acos_det(x)
    worst = 0.0
    for a, b in zip(x.tolist(), y.tolist()):
        aa = 0.0 if a == 0 else a
        assert sim3_literal.atan2_det(math.sqrt((1.0 - aa) * (1.0 + aa)), aa) == b
        true = _acos_true(a, ctx)
        if true is None or true == 0:
            continue
        rel = abs(float((decimal.Decimal(b) - true) / true))
        worst = max(worst, rel)
        assert rel <= lit.ACOS_DET_BOUND, (a, rel / U)
    print("acos_det worst relative error / 2^-53: %.3f" % (worst / U))
    th = np.random.default_rng(5).uniform(-7, 7, 500)
    s, c = lit.sincos_d(th)
    for t, a, b in zip(th.tolist(), s.tolist(), c.tolist()):
        assert sim3_literal.sincos_d(t) == (a, b)


LOG_PROBE_UPDATES = [  # (omega, upsilon, sigma): one per log() branch, + zero, a large rotation, both pivot outcomes
    [1e-4, -2e-4, 3e-4, 0.3, -0.2, 0.5, 2e-6],
    [0.1, -0.2, 0.05, 0.3, -0.2, 0.5, -3e-6],
    [1e-4, -2e-4, 3e-4, 0.3, -0.2, 0.5, 0.05],
    [0.1, -0.2, 0.05, 0.3, -0.2, 0.5, -0.07],
    [0.0] * 7,
    [2.0, 1.5, -1.0, 0.3, 0.2, -0.1, 0.4],
    [0.02, 0.01, 2.4, 1.0, -2.0, 0.5, 0.2],
    [-1.9, 0.3, 0.2, 1.0, 2.0, 3.0, -0.3],
    [0.0, 0.0, 0.0, 1.0, 2.0, 3.0, 0.0],
    [1e-9, 0, 0, 0, 0, 0, 0],
]


def _log_probe_set():
    rng = np.random.default_rng(6)
    U7 = [np.array(u, float) for u in LOG_PROBE_UPDATES]
    for _ in range(60):
        w = rng.normal(0, 1, 3) * rng.choice([1e-4, 0.3, 1.2])
        w *= min(1.0, 2.7 / np.linalg.norm(w))  # log() returns the rotation below pi
        U7.append(np.concatenate([w, rng.normal(0, 2, 3), [rng.choice([0.0, 1e-7, 0.2, -0.4])]]))
    return U7


def test_sim3_log_inverts_exp():
    """log(exp(u)) returns u and exp(log(S)) returns S.

    Tolerances.  In the d > 1 - eps branch the reference takes omega = 0.5*deltaR(R) = sin(theta) * axis for
    theta * axis: a design error of theta^3 / 6 with theta < sqrt(2 eps) = 4.5e-3, i.e. up to 1.5e-8, which
    also enters upsilon through W (|dW| <= theta^3/6 * (A + ...) < the same, times |t| <= 8): 2e-8 resp.
    2e-7.  Elsewhere the error is rounding: d is formed from R's entries, each within ~8u, and theta =
    acos(d) has d theta = dd / sin(theta) with sin(theta) >= 4.4e-3 in this branch, so |d theta| <= 8u /
    4.4e-3 + 20u * pi (ACOS_DET_BOUND) = 2.1e-13; omega = theta/(2 sqrt(1-d^2)) * deltaR divides a second
    time by sin(theta): 5e-11 at worst near the branch point and 1e-13 for theta >= 0.05, the smallest
    rotation of this probe set outside the first branch; sigma carries LOG_DET_BOUND and EXP_DET_BOUND:
    8.5u.  upsilon = W^-1 t with cond(W) < 10 for |omega| <= 2.7, |sigma| <= 0.4: 1e-12.  Asserted: 1e-12 on
    all of u outside the small-rotation branch, 2e-8 (omega) and 2e-7 (upsilon) inside it -- plus, where
    |sigma| >= eps there, the reference's own B: `((0.5*sigma2-sigma+1)*s)/(sigma2*sigma)` lacks the "- 1" of
    the limit it stands for (the same line in the constructor, where theta < 1e-5 hides it), so W is off by
    about theta^2 * |B_ref| and upsilon by that times |upsilon|; the restatement keeps the line as it is."""
    seen = collections.Counter()
    for u in _log_probe_set():
        S = osl.sim3_exp(list(u))
        r, br = lit.sim3_log(S, seen, want_branch=True)
        r = np.array([float(v) for v in r])
        if int(br) & 1:
            assert np.abs(r - u).max() <= 1e-12, (u, r)
            tol = 1e-12
        else:
            sg, th2 = u[6], float(u[:3] @ u[:3])
            b_ref = abs((0.5 * sg * sg - sg + 1) * math.exp(sg) / sg ** 3) if abs(sg) >= 0.00001 else 0.0
            tol = 2e-7 + 2 * th2 * (b_ref + 1 / 6) * float(np.linalg.norm(u[3:6]))
            assert np.abs(r[:3] - u[:3]).max() <= 2e-8 and np.abs(r[3:6] - u[3:6]).max() <= tol, (u, r)
            assert abs(r[6] - u[6]) <= 1e-15
        S2 = osl.sim3_exp(list(r))
        assert np.abs(osl.sim3_to8(S2) - osl.sim3_to8(S)).max() <= tol
    for b in lit.LOG_BRANCHES:
        assert seen[b] > 0, b
    assert seen["lu_swap_first"] > 0 and seen["lu_swap_second"] > 0 and seen["lu_no_swap"] > 0
    # scale exactly 1: sigma exactly 0, the |sigma| < eps branch
    r, br = lit.sim3_log(osl.sim3_exp([0.3, 0.1, -0.2, 1.0, 2.0, 3.0, 0.0]), want_branch=True)
    assert float(r[6]) == 0.0 and int(br) & 2 == 0


# ------------------------------------------------------------------ CPU: Jacobians, the solve
def _closed_form_jacobians(C, v0, v1):
    """d log(C * exp(u0) v0 * (exp(u1) v1)^-1) / du at 0 by the adjoint: with E = C v0 v1^-1 and e = log E,
    exp(e + de) = C exp(u0) v0 v1^-1 exp(-u1); to first order de = Jl^-1(e) (Ad_C u0 - Ad_E u1), Jl the left
    Jacobian of Sim(3).  Both Ad and Jl^-1 are formed numerically from 7x7 matrix exponentials / logarithms
    of the generators in numpy (scipy-free): Jl^-1(e) = sum_k B_k ad_e^k / k! (Bernoulli series, |e| small)."""
    def hat(u):
        w, v, s = u[:3], u[3:6], u[6]
        M = np.zeros((4, 4))
        M[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + s * np.eye(3)
        M[:3, 3] = v
        return M

    def vee(M):
        return np.array([M[2, 1], M[0, 2], M[1, 0], M[0, 3], M[1, 3], M[2, 3], M[0, 0]])

    def mat(S):
        q, t, s = S
        R = np.array(lit.qmat(tuple(float(a) for a in q)), float).reshape(3, 3)
        M = np.eye(4)
        M[:3, :3] = float(s) * R
        M[:3, 3] = [float(a) for a in t]
        return M

    def Ad(T):
        Ti = np.linalg.inv(T)
        return np.stack([vee(T @ hat(np.eye(7)[k]) @ Ti) for k in range(7)], axis=1)

    def ad(e):
        return np.stack([vee(hat(e) @ hat(np.eye(7)[k]) - hat(np.eye(7)[k]) @ hat(e)) for k in range(7)], axis=1)
    TC, T0, T1 = mat(C), mat(v0), mat(v1)
    TE = TC @ T0 @ np.linalg.inv(T1)
    e = np.array([float(v) for v in lit.sim3_log(sim3_of(TE))])
    a = ad(e)
    bern = [1.0, -0.5, 1 / 6, 0.0, -1 / 30, 0.0, 1 / 42, 0.0, -1 / 30]
    Jli, P, f = np.zeros((7, 7)), np.eye(7), 1.0
    for k, bk in enumerate(bern):
        if k:
            P, f = P @ a, f * k
        Jli += bk / f * P
    return Jli @ Ad(TC), -Jli @ Ad(TE)


def sim3_of(T):
    s = float(np.cbrt(np.linalg.det(T[:3, :3])))
    return osl.sim3_from8(osl.sim3_from_rts(T[:3, :3] / s, T[:3, 3], s))


def test_numeric_jacobian_against_the_closed_form():
    """The literal's central differences against the closed-form Jacobian of EdgeSim3's error at 12 random
    states with an error of up to ~0.1 in each entry.

    Margin from delta = 1e-9: the error entries are O(0.1..1) doubles, each evaluated through ~100 roundings:
    |noise| <= ~50u * 1 = 6e-15 per evaluation, the difference of two divided by 2 delta: 6e-6 absolute at
    the very worst, 1e-6 typical; the central difference's truncation is delta^2 * f''' / 6 ~ 1e-18:
    nothing.  The Jacobian entries are O(1) (adjoints of poses with |t| <= 3).  Asserted: 2e-5 absolute, a
    little over the worst-case noise, four orders below the entries' size."""
    rng = np.random.RandomState(21)
    worst = 0.0
    for _ in range(12):
        def rnd(scale):
            return osl.sim3_exp(list(np.concatenate([rng.normal(0, scale, 3), rng.normal(0, 1.0, 3),
                                                     [rng.normal(0, 0.1)]])))
        v0, v1 = rnd(0.8), rnd(0.8)
        Cm = osl.sim3_mul(osl.sim3_mul(osl.sim3_exp(list(rng.normal(0, 0.05, 7))), v1), osl.sim3_inverse(v0))
        P = {"Scw": np.array([osl.sim3_to8(v0), osl.sim3_to8(v1), osl.sim3_to8(v1)]), "edge_v0": [0], "edge_v1": [1],
             "edge_kind": [0], "fixed_vertex": 2, "bFixScale": False}
        P["Snc"] = P["Scw"]
        G = lit.Graph(P, collections.Counter())
        G.meas = osl.sim3_to8(Cm).reshape(1, 8)
        G.C = lit.sim3_cols(G.meas)
        J0, J1 = G.jacobians()
        A0, A1 = _closed_form_jacobians(Cm, v0, v1)
        worst = max(worst, np.abs(J0[0] - A0).max(), np.abs(J1[0] - A1).max())
        assert np.abs(A0).max() > 0.5
    print("numeric Jacobian worst absolute deviation: %.3e" % worst)
    assert worst <= 2e-5


def test_ldlt_solve_against_numpy():
    """The literal's LDL^T solve of the scenes' own H + lambda I against numpy.linalg.solve.

    Condition numbers observed on the scenes' first systems (printed below): 1e4 .. 2e5 for the coupled
    unknowns.  Under bFixScale every scale unknown has an exactly zero row, column and right-hand side (its
    Jacobian column is zero), so H + lambda I carries lambda alone there, x is exactly 0 and the 1e18 that
    numpy.linalg.cond reports for the whole matrix at lambda = 1e-16 says nothing about the rest: the
    figure is taken without those rows.  A backward-stable solve is within ~N * cond * u = 273 * 2e5 *
    1.1e-16 = 6e-9 relative, and so is numpy's: asserted 2e-8 relative to max |x|."""
    for name in scenes.CASES:
        G = scenes.case(name)[1]["graph"]
        for lam in (1e-16, 1e-3):
            ok, x = lit.ldlt_solve(G.H0, G.b0, lam)
            A = G.H0 + lam * np.eye(G.N)
            want = np.linalg.solve(A, G.b0)
            assert ok
            live = np.flatnonzero(np.diag(G.H0) != 0.0)
            cond = np.linalg.cond(A[np.ix_(live, live)])
            print("%s lambda %g: cond %.2e, deviation %.2e" % (name, lam, cond, np.abs(x - want).max() / np.abs(want).max()))
            assert cond <= 2e5
            assert np.abs(x - want).max() <= 2e-8 * np.abs(want).max()
            dead = np.setdiff1d(np.arange(G.N), live)
            assert (len(dead) > 0) == bool(G.fix) and np.all(x[dead] == 0.0)
    ok, _ = lit.ldlt_solve(np.zeros((7, 7)), np.ones(7), 0.0)
    assert ok is False
    Z = np.eye(7)
    Z[3, 3] = 0.0
    assert lit.ldlt_solve(Z, np.ones(7), 0.0)[0] is False and lit.ldlt_solve(Z, np.ones(7), 1e-3)[0] is True


# ------------------------------------------------------------------ CPU: the scenes
def _position_errors(M, r):
    """|camera centre - truth| before and after, in the metric of the loop keyframe's side (the centres of
    the optimised Sim3s: -R^T t / s)."""
    before, after = [], []
    for kf in M["keyframes"]:
        if kf["bad"]:
            continue
        i = kf["id"]
        Tt = M["truth"][i]
        c_true = -Tt[:3, :3].T @ Tt[:3, 3]
        Te = np.asarray(kf["Tcw"], float)
        before.append(np.linalg.norm(-Te[:3, :3].T @ Te[:3, 3] - c_true))
        To = np.asarray(r["Tcw"][i], float)
        after.append(np.linalg.norm(-To[:3, :3].T @ To[:3, 3] - c_true))
    return np.array(before), np.array(after)


@pytest.mark.parametrize("name", list(scenes.CASES))
def test_literal_converges_and_closes_the_ring(name):
    """chi2 drops, the break in the ring is spread, and the ring closes at pCurKF to within the injected
    noise: its camera centre ends within 3 * n * sqrt 3 * (STEP_TRANS + RADIUS * STEP_ROT) of the truth
    (three sigma of the odometry noise had it all accumulated one way round the ring), where at n >= 12 the
    drifted estimate (yaw and scale bias) missed it by more than three times what is left."""
    M, r = scenes.case(name)
    n = sum(1 for kf in M["keyframes"] if not kf["bad"])
    assert r["chi2_final"] < r["chi2_initial"] and r["iterations"] >= 1 and r["solver_failures"] == 0
    G = r["graph"]
    G1 = lit.Graph(r["problem"], collections.Counter())
    G1.est = r["Scw_out"].copy()
    res0, res1 = np.linalg.norm(G.err0, axis=1).max(), np.linalg.norm(G1.errors(), axis=1).max()
    if n >= 12:
        # the loop error e sits at first on the k <= 5 edges that join corrected and uncorrected keyframes
        # (chi2 ~ k (e/k)^2) and ends spread over the ring's n edges (~ e^2 / n): a drop by about n / k >= 2.4
        assert r["chi2_final"] <= 0.5 * r["chi2_initial"], (r["chi2_initial"], r["chi2_final"])
        assert res1 <= 0.5 * res0, (res0, res1)
    if n >= 3:
        cur = M["pCurKF"]

        def centre(T):
            T = np.asarray(T, float)
            return -T[:3, :3].T @ T[:3, 3]
        c_true = centre(M["truth"][cur])
        before = np.linalg.norm(centre([kf for kf in M["keyframes"] if kf["id"] == cur][0]["Tcw"]) - c_true)
        after = np.linalg.norm(centre(r["Tcw"][cur]) - c_true)
        bound = 3 * n * math.sqrt(3) * (scenes.STEP_TRANS + scenes.RADIUS * scenes.STEP_ROT)
        print("%s: pCurKF centre error before %.4f after %.4f (bound %.4f), largest edge residual %.4f -> %.4f, "
              "chi2 %.3e -> %.3e, %d its %d trials" % (name, before, after, bound, res0, res1, r["chi2_initial"],
                                                      r["chi2_final"], r["iterations"], r["trials"]))
        assert after <= bound
        if n >= 12:
            assert before > 3 * after
    if M["bFixScale"]:
        assert np.array_equal(_bits(r["Scw_out"][:, 7]), _bits(r["problem"]["Scw"][:, 7]))  # s * exp_det(0)
    bad_pts = [k for k, mp in enumerate(M["points"]) if mp["bad"]]
    assert bad_pts and all(k not in r["pos"] for k in bad_pts) and len(r["pos"]) == len(M["points"]) - len(bad_pts)


def test_scene_set_reaches_every_branch():
    """The literal's counters over the scene set (conditions on the scenes, checked here before any GPU
    run): every log() branch and both LU pivot outcomes inside the optimisation, a rejected LM trial, the
    20-iteration cap or a stop rule, the duplicate-pair block, a transposed block, the fix_scale zeroing,
    the minFeat exception and a sInsertedEdges skip."""
    total = collections.Counter()
    for name in scenes.CASES:
        total.update(scenes.case(name)[1]["counters"])
    print(dict(total))
    for b in lit.LOG_BRANCHES:
        assert total[b] > 0, b
    assert total["lu_no_swap"] > 0 and total["lu_swap_first"] + total["lu_swap_second"] > 0
    for k in ("rejected_trials", "duplicate_pair_block", "transposed_block", "fix_scale_zeroing",
              "minfeat_exception", "inserted_edges_skip"):
        assert total[k] > 0, k
    assert total["iteration_cap"] + total["stop_rule"] == len(scenes.CASES)
    sizes = {len(scenes.case(n)[1]["problem"]["vertex_id"]) for n in scenes.CASES}
    assert sizes == {2, 3, 12, 40}
    assert scenes.case("n40_free")[1]["graph"].N == 273
    assert len(scenes.case("n2_fix")[1]["problem"]["edge_v0"]) == 1


def test_python_edge_selection_against_the_hand_listed_set():
    """orb.py's edge selection on the n = 12 scene equals the hand-listed edges (order included), and equals
    the literal's own selection on every scene."""
    from orb_slam2_commit_amd.orb import essential_graph_edges
    M = scenes.case("n12_free")[0]
    assert essential_graph_edges(M) == scenes.EXPECTED_N12
    for name in scenes.CASES:
        M = scenes.case(name)[0]
        assert essential_graph_edges(M) == lit.select_edges(M), name


def test_struct_sizes_and_argument_checks():
    """The new structs are registered in orbx_sizeof and the argument check refuses bad graphs before any
    device call (no GPU needed: the check runs first)."""
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd.orb import essential_graph_structs
    L = _lib.lib()
    assert L.orbx_sizeof(b"orbx_essential_graph_problem") == C.sizeof(_lib.EssGraphProblem)
    assert L.orbx_sizeof(b"orbx_essential_graph_result") == C.sizeof(_lib.EssGraphResult)
    base = scenes.case("n3_fix")[1]["problem"]

    def status(**kw):
        P = dict(base)
        for k, v in kw.items():
            P[k] = v
        p, r, _ = essential_graph_structs(P)
        return L.orbx_optimize_essential_graph(C.byref(p), C.byref(r), 0)
    assert status(edge_v0=np.array([5, 2, 2], np.int32)[:len(base["edge_v0"])]) == _lib.ORBX_ERR_ARG
    same = base["edge_v1"].copy()
    assert status(edge_v0=same) == _lib.ORBX_ERR_ARG                                 # v0 == v1
    assert status(vertex_id=np.array([0, 2, 1], np.int32)) == _lib.ORBX_ERR_ARG     # not ascending
    assert status(fixed_vertex=3) == _lib.ORBX_ERR_ARG
    assert status(lambda_init=0.0) == _lib.ORBX_ERR_ARG
    bad_ref = base["point_ref"].copy()
    bad_ref[0] = 3
    assert status(point_ref=bad_ref) == _lib.ORBX_ERR_ARG
    one = dict(base, vertex_id=base["vertex_id"][:1], Scw=base["Scw"][:1], Snc=base["Snc"][:1], fixed_vertex=0,
               edge_v0=base["edge_v0"][:0], edge_v1=base["edge_v1"][:0], edge_kind=base["edge_kind"][:0],
               Xw=base["Xw"][:0], point_ref=base["point_ref"][:0])
    p, r, _ = essential_graph_structs(one)
    assert L.orbx_optimize_essential_graph(C.byref(p), C.byref(r), 0) == _lib.ORBX_ERR_ARG  # n_vertices < 2
    T = np.ascontiguousarray(scenes.case("n3_fix")[0]["keyframes"][1]["Tcw"], np.float32)
    out = np.zeros(8)
    L.orbx_sim3_from_tcw(_lib.ptr(T), _lib.ptr(out))
    assert np.array_equal(_bits(out), _bits(lit.sim3_from_tcw(T)))


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_log_det_and_acos_det_grids(gpu):
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd._lib import ptr
    for fn, x, twin in (("orbx_debug_log", _log_grid(), lit.log_det), ("orbx_debug_acos", _acos_grid(), lit.acos_det)):
        x = np.ascontiguousarray(x[np.isfinite(twin(x))])
        y = np.zeros_like(x)
        _lib.check(getattr(_lib.lib(), fn)(ptr(x), len(x), ptr(y), 0), fn)
        assert np.array_equal(_bits(y), _bits(twin(x))), fn


@pytest.mark.gpu
def test_gpu_sim3_log_probe_covers_every_branch(gpu):
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd._lib import ptr
    S = np.array([osl.sim3_to8(osl.sim3_exp(list(u))) for u in _log_probe_set()])
    out, br = np.zeros((len(S), 7)), np.zeros(len(S), np.int32)
    _lib.check(_lib.lib().orbx_debug_sim3_log(ptr(S), len(S), ptr(out), ptr(br), 0), "orbx_debug_sim3_log")
    want, wbr = lit.sim3_log(lit.sim3_cols(S), want_branch=True)
    assert np.array_equal(br, wbr.astype(np.int32))
    assert np.array_equal(_bits(out), _bits(np.stack(want, axis=1)))
    assert {0, 1, 2, 3} <= set((br & 3).tolist()) and (br & 4).any() and (br & 8).any() and ((br & 12) == 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(scenes.CASES))
def test_gpu_first_linearisation_bit_exact(gpu, name):
    """orbx_debug_essgraph_linearize: measurements, errors, both Jacobians per edge, H and b."""
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd._lib import ptr
    from orb_slam2_commit_amd.orb import essential_graph_structs
    r = scenes.case(name)[1]
    P, G = r["problem"], r["graph"]
    E, N = G.E, G.N
    p, _, _ = essential_graph_structs(P)
    meas, err, J0, J1 = np.zeros((E, 8)), np.zeros((E, 7)), np.zeros((E, 7, 7)), np.zeros((E, 7, 7))
    H, b = np.zeros((N, N)), np.zeros(N)
    _lib.check(_lib.lib().orbx_debug_essgraph_linearize(C.byref(p), ptr(meas), ptr(err), ptr(J0), ptr(J1), ptr(H),
                                                        ptr(b), 0), "orbx_debug_essgraph_linearize")
    G0 = lit.Graph(P, collections.Counter())
    e0 = G0.errors()
    G0.build(e0)
    assert np.array_equal(_bits(meas), _bits(G0.meas))
    assert np.array_equal(_bits(err), _bits(e0))
    assert np.array_equal(_bits(J0), _bits(G0.J0)) and np.array_equal(_bits(J1), _bits(G0.J1))
    assert np.array_equal(_bits(b), _bits(G0.b))
    assert np.array_equal(_bits(H + 0.0), _bits(G0.H + 0.0))  # (+ 0.0: a structural zero has no sign)
    assert np.array_equal(_bits(G0.H), _bits(G.H0))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(scenes.CASES))
def test_gpu_solve_probe_bit_exact(gpu, name):
    """orbx_debug_essgraph_solve on the scene's first system at two lambdas, and the zero-pivot verdict."""
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd._lib import ptr
    from orb_slam2_commit_amd.orb import essential_graph_structs
    r = scenes.case(name)[1]
    P, G = r["problem"], r["graph"]
    p, _, _ = essential_graph_structs(P)
    for lam in (1e-16, 1e-3):
        x, ok = np.zeros(G.N), np.zeros(1, np.int32)
        _lib.check(_lib.lib().orbx_debug_essgraph_solve(C.byref(p), ptr(G.H0), ptr(G.b0), lam, ptr(x), ptr(ok), 0),
                   "orbx_debug_essgraph_solve")
        okl, xl = lit.ldlt_solve(G.H0, G.b0, lam)
        assert ok[0] == 1 and okl
        assert np.array_equal(_bits(x), _bits(xl)), np.abs(x - xl).max()
    Z = np.ascontiguousarray(G.H0.copy())
    Z[:7, :] = 0.0
    Z[:, :7] = 0.0
    x, ok = np.zeros(G.N), np.zeros(1, np.int32)
    _lib.check(_lib.lib().orbx_debug_essgraph_solve(C.byref(p), ptr(Z), ptr(G.b0), 0.0, ptr(x), ptr(ok), 0), "zero pivot")
    assert ok[0] == 0 and lit.ldlt_solve(Z, G.b0, 0.0)[0] is False


def _same_run(g, o):
    assert g["iterations"] == o["iterations"] and g["trials"] == o["trials"], (g["iterations"], g["trials"],
                                                                                 o["iterations"], o["trials"])
    assert g["solver_failures"] == o["solver_failures"]
    assert _bits(g["chi2_initial"]) == _bits(o["chi2_initial"]) and _bits(g["chi2_final"]) == _bits(o["chi2_final"])
    assert np.array_equal(_bits(g["Scw_out"]), _bits(o["Scw_out"]))
    assert np.array_equal(np.ascontiguousarray(g["Tcw_out"]).view(np.uint32), o["Tcw_out"].view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(g["Xw_out"]).view(np.uint32), o["Xw_out"].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(scenes.CASES))
def test_gpu_optimize_essential_graph_bit_exact(gpu, name):
    from orb_slam2_commit_amd import Optimizer
    M, o = scenes.case(name)
    opt = Optimizer()
    g = opt.OptimizeEssentialGraph(M)
    opt.close()
    raw = dict(g["raw"], iterations=g["iterations"], trials=g["trials"], solver_failures=g["solver_failures"],
               chi2_initial=g["chi2_initial"], chi2_final=g["chi2_final"])
    _same_run(raw, o)
    assert set(g["Tcw"]) == set(o["Tcw"]) and set(g["pos"]) == set(o["pos"])
    for i in o["Tcw"]:
        assert np.array_equal(g["Tcw"][i].view(np.uint32), o["Tcw"][i].view(np.uint32))
    for k in o["pos"]:
        assert np.array_equal(g["pos"][k].view(np.uint32), o["pos"][k].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n3_free", "n40_fix"])
def test_gpu_device_form_equals_the_host_form(gpu, name):
    """orbx_optimize_essential_graph_device on torch's current stream, device-resident pose tables, points
    and outputs: the literal's bits (hence the host form's)."""
    import torch
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd.orb import essential_graph_structs
    o = scenes.case(name)[1]
    P = dict(o["problem"])
    n, m = len(P["vertex_id"]), len(P["point_ref"])
    for k in ("Scw", "Snc", "Xw", "point_ref"):
        P[k] = torch.from_numpy(np.ascontiguousarray(P[k])).to(gpu)
    outs = dict(Scw_out=torch.zeros((n, 8), dtype=torch.float64, device=gpu),
                Tcw_out=torch.zeros((n, 12), dtype=torch.float32, device=gpu),
                Xw_out=torch.zeros((m, 3), dtype=torch.float32, device=gpu),
                iterations=torch.zeros(1, dtype=torch.int32, device=gpu),
                trials=torch.zeros(1, dtype=torch.int32, device=gpu),
                chi2_initial=torch.zeros(1, dtype=torch.float64, device=gpu),
                chi2_final=torch.zeros(1, dtype=torch.float64, device=gpu),
                solver_failures=torch.zeros(1, dtype=torch.int32, device=gpu))
    p, r, _ = essential_graph_structs(P, outs)
    s = torch.cuda.current_stream()
    _lib.check(_lib.lib().orbx_optimize_essential_graph_device(C.byref(p), C.byref(r), C.c_void_p(s.cuda_stream)),
               "orbx_optimize_essential_graph_device")
    torch.cuda.synchronize()
    g = {k: v.cpu().numpy() for k, v in outs.items()}
    for k in ("iterations", "trials", "solver_failures"):
        g[k] = int(g[k][0])
    for k in ("chi2_initial", "chi2_final"):
        g[k] = float(g[k][0])
    _same_run(g, o)
