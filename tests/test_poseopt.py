"""Optimizer::PoseOptimization (src/Optimizer.cc:287-528).

CPU: the oracle's OnlyPose Jacobians against central finite differences, its
Eigen-LDLT restatement against numpy, convergence / outlier-rejection KATs and
the reference's early exits; the literal restatement (tests/poseopt_literal.py)
against the oracle BIT FOR BIT on the case table of tests/poseopt_scenes.py, the
table's branch counters, the literal's sums against exact arithmetic and its
Jacobian rows against central differences.  GPU (-m gpu): the HIP kernel (one
block per frame, whole four-round schedule on the device) against the oracle
and against the literal BIT FOR BIT -- pose as float bits, outlier flags, return
value and the LM iteration count of every round -- on single frames, on device
batches (device-resident sizes and start poses included) and on one handle
called with large and small problems in turn.
Parity vs the genuine g2o/Eigen binary is unpinned.
"""
import collections
import fractions
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle  # noqa: E402
import poseopt_literal as lit  # noqa: E402
import poseopt_scenes as scenes  # noqa: E402
from orb_slam2_commit_amd import synth  # noqa: E402


def _rotmat_to_q(R):
    from scipy.spatial.transform import Rotation
    x, y, z, w = Rotation.from_matrix(R).as_quat()
    return np.array([x, y, z, w])


@pytest.mark.parametrize("stereo", [0, 1])
def test_onlypose_jacobian_finite_differences(stereo):
    rng = np.random.default_rng(stereo)
    intr = np.array([718.856, 718.856, 607.1928, 185.2157, 386.1448])
    for _ in range(20):
        from scipy.spatial.transform import Rotation
        R = Rotation.from_rotvec(rng.normal(0, 0.3, 3)).as_matrix()
        q = _rotmat_to_q(R)
        t = rng.normal(0, 1, 3)
        Xc = np.array([rng.uniform(-5, 5), rng.uniform(-2, 2), rng.uniform(3, 30)])
        X = R.T @ (Xc - t)
        obs = np.array([600.0, 180.0, 500.0])
        e0, J = oracle.pose_edge_probe(q, t, X, intr, stereo, obs)
        D = 3 if stereo else 2
        h = 1e-3 if stereo else 1e-6  # invz is float-rounded in the stereo cam_project
        Jn = np.zeros((D, 6))
        for k in range(6):
            u = np.zeros(6)
            u[k] = h
            qp, tp = oracle.se3_exp_mul(u, q, t)
            u[k] = -h
            qm, tm = oracle.se3_exp_mul(u, q, t)
            ep, _ = oracle.pose_edge_probe(qp, tp, X, intr, stereo, obs)
            em, _ = oracle.pose_edge_probe(qm, tm, X, intr, stereo, obs)
            Jn[:, k] = (ep[:D] - em[:D]) / (2 * h)  # _jacobianOplusXi = d error / d update
        scale = np.abs(J[:D]).max()
        np.testing.assert_allclose(J[:D], Jn, atol=(5e-3 if stereo else 1e-6) * scale)


def test_ldlt6_against_numpy():
    rng = np.random.default_rng(0)
    for _ in range(50):
        A = rng.normal(0, 1, (6, 6))
        H = A @ A.T + 0.1 * np.eye(6)
        H[np.arange(6), np.arange(6)] *= rng.uniform(0.1, 1e4, 6)  # forces diagonal pivoting
        b = rng.normal(0, 1, 6)
        ok, x = oracle.ldlt6(H, b)
        assert ok
        assert np.allclose(x, np.linalg.solve(H, b), rtol=1e-8, atol=1e-10)
    ok, _ = oracle.ldlt6(-np.eye(6) + 0.01 * np.ones((6, 6)), np.ones(6))
    assert not ok  # !isPositive(): LM rejects the step
    ok, x = oracle.ldlt6(np.zeros((6, 6)), np.ones(6))  # ZeroSign: isPositive, solution 0
    assert ok and np.all(x == 0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_converges_and_rejects_outliers(seed):
    pr = synth.pose_problem(seed, n=800)
    o = oracle.pose_optimization(pr)
    Tt = pr["Ttrue"]
    err0 = np.abs(pr["Tcw"][:3, 3] - Tt[:3, 3]).max()
    err1 = np.abs(o["Tcw"][:3, 3] - Tt[:3, 3]).max()
    assert err1 < 0.1 * err0 and err1 < 5e-3
    gross = pr["is_outlier"]
    assert o["outlier"][gross].mean() > 0.95  # gross outliers flagged
    assert o["ngood"] == len(gross) - int(o["outlier"].sum())
    assert all(1 <= k <= 10 for k in o["iterations"])


def test_oracle_early_exits():
    pr = synth.pose_problem(4, n=2)
    o = oracle.pose_optimization(pr)  # nInitialCorrespondences < 3: return 0, pose untouched
    assert o["ngood"] == 0 and np.array_equal(o["Tcw"], pr["Tcw"]) and (o["iterations"] == 0).all()
    pr = synth.pose_problem(4, n=8)
    o = oracle.pose_optimization(pr)  # < 10 edges: one round only
    assert o["iterations"][0] > 0 and (o["iterations"][1:] == 0).all()


# ------------------------------------------------------------------ CPU: the literal restatement
def _same_result(a, b):
    """Two yardsticks' results agree bit for bit."""
    assert a["ngood"] == b["ngood"], (a["ngood"], b["ngood"])
    assert np.array_equal(a["iterations"], b["iterations"]), (a["iterations"], b["iterations"])
    assert np.array_equal(a["outlier"], b["outlier"])
    assert np.array_equal(a["Tcw"].view(np.uint32), b["Tcw"].view(np.uint32)), (a["Tcw"], b["Tcw"])


def test_huber_deltas_agree():
    """src/Optimizer.cc:324-325 rounds a double square root to float; the oracle and the kernel take the
    float square root of the float constant.  Both are the same float for both constants."""
    dm, ds = lit.huber_deltas()
    assert dm == float(np.sqrt(np.float32(5.991))) and ds == float(np.sqrt(np.float32(7.815)))


@pytest.mark.parametrize("name", list(scenes.CASES))
def test_literal_equals_oracle_on_the_case_table(name):
    P, r = scenes.case(name)
    _same_result(r, oracle.pose_optimization(P))


def test_literal_equals_oracle_on_the_batch():
    batch = scenes.batch_problems()
    assert len(batch) == 24
    for e in batch:
        r = lit.pose_optimization(e["effective"])
        _same_result(r, oracle.pose_optimization(e["effective"]))
        if e["n_dev"] is not None:  # the clamp min(max(n_dev, 0), capacity), and a host pose that differs
            cap = len(e["problem"]["obs"])
            assert len(e["effective"]["obs"]) == min(max(e["n_dev"], 0), cap)
            assert cap - len(e["effective"]["obs"]) in ((1, 64, 300) if 0 <= e["n_dev"] <= cap else (0, cap))
            assert not np.array_equal(e["problem"]["Tcw"], e["Tcw_dev"])
            assert np.array_equal(e["effective"]["Tcw"], e["Tcw_dev"])
    sizes = [len(e["effective"]["obs"]) for e in batch]
    assert {0, 2, 3, 9, 10, 257} <= set(sizes) and min(sizes[k] for k in range(0, 24, 3)) < 10
    assert sum(e["n_dev"] is not None for e in batch) == 8
    assert any(e["n_dev"] is not None and e["n_dev"] > len(e["problem"]["obs"]) for e in batch)
    assert any(e["n_dev"] == -5 for e in batch)


def test_case_table_reaches_every_branch():
    """The literal's counters over the case table: every key of lit.COUNTERS fires somewhere except the failed
    solve (H is a sum of positive-semidefinite terms and lambda > 0, so isPositive() cannot fail on finite
    inputs), each named case reports what the table says of it, the first round's active list sits on every
    wave, chunk and pass edge, and a two-pass trial-chi round occurs in a later round too.

    round_ended_on_rejected_trial proves the classification runs on a rejected trial's errors (17 rounds of
    the table).  It does not make that rule observable: the loop leaves a rejected trial only on rho == 0 or
    on the tenth trial, when the step has shrunk to nothing -- over the table the stale errors differ from the
    restored pose's by at most 5.6e-8 px, far below what the float chi2 resolves at the threshold, and a
    literal that recomputes them gives the same results on every case."""
    total = collections.Counter()
    for name in scenes.CASES:
        total.update(scenes.case(name)[1]["counters"])
    for k in lit.COUNTERS:
        if k == "solve_not_positive":
            assert total[k] == 0
        else:
            assert total[k] > 0, k
    assert set(scenes.REQUIRED) == set(lit.COUNTERS) - {"solve_not_positive", "mat2q_trace"}
    for k, names in scenes.REQUIRED.items():
        for name in names:
            assert scenes.case(name)[1]["counters"][k] > 0, (k, name)
    assert {scenes.case(n)[1]["nact"][0] if len(scenes.case(n)[0]["obs"]) >= 3 else len(scenes.case(n)[0]["obs"])
            for n in scenes.CASES} >= set(scenes.NACT0)
    r = scenes.case("n7425")[1]
    assert r["nact"][0] == scenes.CHI_PASS + 1 and max(r["nact"][1:]) <= scenes.CHI_PASS
    assert min(scenes.case("n8200_out0")[1]["nact"]) > scenes.CHI_PASS
    for name in ("n255_out30", "n257_out30", "n513_out30"):  # later rounds fall inside a chunk
        nact = scenes.case(name)[1]["nact"]
        assert all(0 < a < nact[0] and a % 256 for a in nact[1:]), (name, nact)
    # the known oracle results the table was built around
    assert list(scenes.case("n12_all_outliers")[1]["iterations"]) == [6, 0, 0, 0]
    assert scenes.case("n12_all_outliers")[1]["ngood"] == 0
    for name in ("copies3", "copies9"):
        assert list(scenes.case(name)[1]["iterations"]) == [4, 0, 0, 0]
    P, r = scenes.case("n100_behind")
    assert len(P["mirrored"]) == 5
    for name in ("n0", "n2"):
        P, r = scenes.case(name)
        assert r["ngood"] == 0 and np.array_equal(r["Tcw"], P["Tcw"]) and r["trials"] == [0, 0, 0, 0]


def _mixed_small(seed, n):
    P = synth.pose_problem(seed, n=n, p_stereo=0.5, outlier_frac=0.25)
    st = P["obs"][:, 2] >= 0
    assert 0 < st.sum() < n  # mono and stereo mixed
    return P


@pytest.mark.parametrize("robust", [1, 0])
@pytest.mark.parametrize("seed,n", [(31, 12), (32, 40)])
def test_literal_sums_against_exact_arithmetic(seed, n, robust):
    """The first iteration's H, b and chi: the literal's sequential sums against the exact rational sums of
    its own per-edge terms.  A chain of n additions from zero errs by at most (n - 1) u sum|term| to first
    order (u = 2^-53); the assertion is n u sum|term| per entry.  The first trial's step (accepted: its chi
    is lower) against numpy.linalg.solve at the tolerance test_ldlt6_against_numpy uses."""
    P = _mixed_small(seed, n)
    s = lit.linear_step(P, robust)
    if robust:
        assert any(c > 5.991 for c in s["chi_terms"])  # some edge in Huber's outer region
    F = fractions.Fraction
    u = F(1, 2 ** 53)

    def check(got, terms, sign):
        exact = sign * sum(F(t) for t in terms)
        bound = n * u * sum(abs(F(t)) for t in terms)
        assert abs(F(got) - exact) <= bound, (got, float(exact), float(bound))
    k = 0
    for r in range(6):
        for c in range(r, 6):
            assert s["H"][6 * r + c] == s["H"][6 * c + r]
            check(s["H"][6 * r + c], s["terms"][k], 1)
            k += 1
    for r in range(6):
        check(s["b"][r], s["terms"][21 + r], -1)
    check(s["chi"], s["chi_terms"], 1)
    assert all(len(t) == n for t in s["terms"]) and len(s["terms"]) == 27
    H = np.array(s["H"]).reshape(6, 6) + s["lam"] * np.eye(6)
    assert s["ok"] and s["lam"] == 1e-5 * max(abs(s["H"][7 * j]) for j in range(6))
    assert np.allclose(s["x"], np.linalg.solve(H, np.array(s["b"])), rtol=1e-8, atol=1e-10)
    assert s["temp_chi"] < s["chi"]


@pytest.mark.parametrize("stereo", [0, 1])
def test_literal_jacobian_finite_differences(stereo):
    """The literal's Jacobian rows against central differences of its own error, with the steps and
    tolerances of test_onlypose_jacobian_finite_differences; and both against the oracle's edge, bit for bit."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(stereo)
    K = [718.856, 718.856, 607.1928, 185.2157, 386.1448]
    err = lit.error_stereo if stereo else lit.error_mono
    for _ in range(20):
        R = Rotation.from_rotvec(rng.normal(0, 0.3, 3)).as_matrix()
        q = lit.qnormalize(tuple(float(v) for v in _rotmat_to_q(R)))
        t = [float(v) for v in rng.normal(0, 1, 3)]
        Xc = np.array([rng.uniform(-5, 5), rng.uniform(-2, 2), rng.uniform(3, 30)])
        X = [float(v) for v in R.T @ (Xc - np.array(t))]
        obs = [600.0, 180.0, 500.0]
        T = (q, t)
        D = 3 if stereo else 2
        J = np.array(lit.jacobian_rows(T, X, K))[:D]
        h = 1e-3 if stereo else 1e-6  # invz is float-rounded in the stereo cam_project
        Jn = np.zeros((D, 6))
        for k in range(6):
            up = [0.0] * 6
            up[k] = h
            ep = err(lit.se3_mul(lit.se3_exp(up), T), X, obs, K)
            up[k] = -h
            em = err(lit.se3_mul(lit.se3_exp(up), T), X, obs, K)
            Jn[:, k] = (np.array(ep) - np.array(em)) / (2 * h)
        scale = np.abs(J).max()
        np.testing.assert_allclose(J, Jn, atol=(5e-3 if stereo else 1e-6) * scale)
        e_o, J_o = oracle.pose_edge_probe(np.array(q), np.array(t), np.array(X), np.array(K), stereo, np.array(obs))
        assert np.array_equal(np.array(err(T, X, obs, K)).view(np.uint64), e_o[:D].view(np.uint64))
        assert np.array_equal(J.view(np.uint64), J_o[:D].view(np.uint64))


# ------------------------------------------------------------------ GPU
def _same(g, o):
    ng, T, outl, its = g
    assert ng == o["ngood"], (ng, o["ngood"])
    assert np.array_equal(its, o["iterations"]), (its, o["iterations"])
    assert np.array_equal(outl, o["outlier"])
    assert np.array_equal(T.view(np.uint32), o["Tcw"].view(np.uint32)), (T, o["Tcw"])


CASES = [dict(seed=10, n=1000), dict(seed=11, n=2000), dict(seed=12, n=300, p_stereo=0.0),
         dict(seed=13, n=300, p_stereo=1.0), dict(seed=14, n=500, outlier_frac=0.45),
         dict(seed=15, n=600, rot_sigma=0.05, t_sigma=0.3), dict(seed=16, n=9), dict(seed=17, n=3),
         dict(seed=18, n=2), dict(seed=19, n=0), dict(seed=20, n=4000)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_s%d" % (c["n"], c["seed"]))
def test_gpu_pose_optimization_bit_exact(gpu, case):
    from orb_slam2_commit_amd import Optimizer
    pr = synth.pose_problem(**case)
    o = oracle.pose_optimization(pr)
    opt = Optimizer()
    _same(opt.PoseOptimization(pr), o)


@pytest.mark.gpu
def test_gpu_pose_optimization_device_batch(gpu):
    import ctypes as C
    import torch
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd.orb import pose_problem_struct

    probs, keep, refs = [], [], []
    for b in range(40):
        pr = synth.pose_problem(100 + b, n=200 + 37 * b, p_stereo=(b % 5) / 4.0)
        refs.append(oracle.pose_optimization(pr))
        d = {k: (torch.from_numpy(np.ascontiguousarray(pr[k])).to(gpu) if k in ("obs", "Xw", "inv_sigma2") else pr[k])
             for k in pr}
        n = len(pr["obs"])
        outs = dict(Tcw_out=torch.zeros(16, dtype=torch.float32, device=gpu),
                    outlier=torch.zeros(n, dtype=torch.uint8, device=gpu),
                    ngood=torch.zeros(1, dtype=torch.int32, device=gpu),
                    iterations=torch.zeros(4, dtype=torch.int32, device=gpu))
        p, _ = pose_problem_struct(d, outs)
        probs.append(p)
        keep.append((d, outs))
    arr = (_lib.PoseProblem * len(probs))(*probs)
    s = torch.cuda.current_stream()
    _lib.check(_lib.lib().orbx_pose_optimization_device(arr, len(probs), C.c_void_p(s.cuda_stream)), "batch")
    torch.cuda.synchronize()
    for (d, outs), o in zip(keep, refs):
        g = (int(outs["ngood"].cpu()[0]), outs["Tcw_out"].cpu().numpy().reshape(4, 4), outs["outlier"].cpu().numpy(),
             outs["iterations"].cpu().numpy())
        _same(g, o)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(scenes.CASES))
def test_gpu_pose_optimization_scene(gpu, name):
    """Every case of the table through Optimizer.PoseOptimization against the literal's cached run."""
    from orb_slam2_commit_amd import Optimizer
    P, r = scenes.case(name)
    opt = Optimizer()
    _same(opt.PoseOptimization(P), r)


SENTINEL = 0xA5


@pytest.mark.gpu
def test_gpu_pose_optimization_scene_batch(gpu):
    """scenes.batch_problems() through one orbx_pose_optimization_device launch, each against its own literal
    run: early-exit blocks beside full ones, device-resident sizes (clamped from above and from below) with
    untouched outlier rows beyond them, and device-resident start poses that replace the host's."""
    import ctypes as C
    import torch
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd.orb import pose_problem_struct

    batch = scenes.batch_problems()
    refs = [lit.pose_optimization(e["effective"]) for e in batch]
    probs, keep = [], []
    for e in batch:
        pr = e["problem"]
        cap = len(pr["obs"])
        d = {k: (torch.from_numpy(np.ascontiguousarray(pr[k])).to(gpu) if k in ("obs", "Xw", "inv_sigma2") else pr[k])
             for k in pr}
        outs = dict(Tcw_out=torch.zeros(16, dtype=torch.float32, device=gpu),
                    outlier=torch.full((cap + 1,), SENTINEL, dtype=torch.uint8, device=gpu),
                    ngood=torch.full((1,), -7, dtype=torch.int32, device=gpu),
                    iterations=torch.full((4,), -7, dtype=torch.int32, device=gpu))
        p, _ = pose_problem_struct(d, outs)
        if e["n_dev"] is not None:
            d["n_dev"] = torch.tensor([e["n_dev"]], dtype=torch.int32, device=gpu)
            d["Tcw_dev"] = torch.from_numpy(np.ascontiguousarray(e["Tcw_dev"], np.float32).reshape(16)).to(gpu)
            p.n_dev, p.Tcw_dev = d["n_dev"].data_ptr(), d["Tcw_dev"].data_ptr()
        probs.append(p)
        keep.append((d, outs))
    arr = (_lib.PoseProblem * len(probs))(*probs)
    s = torch.cuda.current_stream()
    _lib.check(_lib.lib().orbx_pose_optimization_device(arr, len(probs), C.c_void_p(s.cuda_stream)), "batch")
    torch.cuda.synchronize()
    for e, (d, outs), r in zip(batch, keep, refs):
        n = len(e["effective"]["obs"])
        outl = outs["outlier"].cpu().numpy()
        g = (int(outs["ngood"].cpu()[0]), outs["Tcw_out"].cpu().numpy().reshape(4, 4), outl[:n],
             outs["iterations"].cpu().numpy())
        _same(g, r)
        assert (outl[n:] == SENTINEL).all()  # rows beyond the device-sized n are not written
        if e["n_dev"] == -5:
            assert g[0] == 0 and n == 0


@pytest.mark.gpu
def test_gpu_pose_optimization_scene_repeat_one_handle(gpu):
    """The per-call path leases pooled scratch: a stale row of a larger earlier call must not leak into a
    smaller later one.  257, 7425 and a far start on one handle, in that order and then reversed."""
    from orb_slam2_commit_amd import Optimizer
    opt = Optimizer()
    order = ["n257", "n7425", "n300_far"]
    for name in order + order[::-1]:
        P, r = scenes.case(name)
        _same(opt.PoseOptimization(P), r)
