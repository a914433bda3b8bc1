"""Optimizer::GlobalBundleAdjustemnt on the GPU (orbx_ba_run_global, Optimizer.GlobalBundleAdjustemnt) and the
tiled reduced-system LDLT (k_ba_ldlt_tiled_*, ORBX_BA_LDLT_TILED) behind it.

CPU: the entry points exist; the literal restatement (globalba_literal.py) is held to the oracle's linear
step and to the reference's Huber deltas; the scene table (globalba_scenes.py) meets its conditions; a numpy
model of the tiled kernel's arithmetic (64-wide panels, W = L D kept unscaled, the forward solve on an
augmented row, the back solve in z's place) meets the solve's criterion.
GPU: every scene against the literal with LocalBA's criterion (_compare of tests/test_localba.py) plus
point_included; the tiled kernel forced on small scenes; the tiled solve alone against numpy from N = 6 to
3072; the size ceiling; LocalBA untouched."""
import ctypes as C

import numpy as np
import pytest

import globalba_literal as lit
import globalba_scenes as scenes
import localba_dense as dn
import oracle
from test_localba import _compare, small_problem

LDLT_TILED = 3
LM_SCENES = ["mono_init", "loop_small", "robust_outliers", "rejects", "nbad", "orphans", "stopped", "stop_mid",
             "beyond_1024"]


# ---------------------------------------------------------------- CPU
def test_entry_points_are_declared_and_exported():
    from orb_slam2_commit_amd import _lib
    for name in ("orbx_ba_run_global", "orbx_ba_run_global_bool"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)
    from orb_slam2_commit_amd import Optimizer
    assert callable(getattr(Optimizer, "GlobalBundleAdjustemnt"))


def test_call_fails_loudly_without_a_handle_or_device():
    from orb_slam2_commit_amd import Optimizer, _lib
    assert _lib.lib().orbx_ba_run_global(None, None, 5, 1, None, None, None) == _lib.ORBX_ERR_ARG
    if _lib.lib().orbx_device_count() <= 0:
        with pytest.raises(_lib.OrbxError) as e:
            Optimizer(0).GlobalBundleAdjustemnt(scenes.problem("loop_small"))
        assert e.value.code == _lib.ORBX_ERR_NODEV


def test_literal_huber_deltas_are_the_reference_floats():
    assert lit.TH_HUBER_2D == float(np.float32(np.sqrt(5.99)))
    assert lit.TH_HUBER_3D == float(np.float32(np.sqrt(7.815)))
    assert lit.TH_HUBER_2D != lit.LOCAL_DELTAS[0]  # not LocalBundleAdjustment's sqrt(5.991f)


def test_literal_first_linear_step_matches_the_oracle():
    """localba_dense.py's rule: the candidate (here the oracle's linear step, without kernels as loop_small
    runs) within FACTOR times the noise of the literal's two orders, measured in the longdouble system."""
    P = scenes.problem("loop_small")
    f = [lit.first_step(P, robust=False, order=o) for o in (0, 1)]
    G = f[0]["graph"]
    ne = G.ne
    o = oracle.ba_linear_step(P, G.cq, G.ct, G.X, np.ones(ne), np.zeros(ne), f[0]["lam"])
    assert o["ok"] and o["nposes"] == len(G.pose_cam) and o["npts"] == len(G.pt_id)
    assert f[0]["lam"] == f[1]["lam"]
    T = dn.edge_terms(P, G.cq, G.ct, G.X)
    ld = dn.assemble(P, T, np.arange(ne), np.zeros(ne), f[0]["lam"], dn.LD)
    ms = [dn.measures(ld, dict(S=x["S"], bs=x["bs"], eerr=x["err"], xp=x["xp"], xl=x["xl"])) for x in f]
    noise = {q: max(ms[0][q], ms[1][q], dn.FLOOR) for q in dn.QUANTITIES}
    m = dn.measures(ld, dict(S=o["S"], bs=o["bs"], eerr=o["err"], xp=o["xp"], xl=o["xl"]))
    ratios = {q: m[q] / noise[q] for q in dn.QUANTITIES}
    dn.report("oracle vs literal, loop_small", ratios)
    assert max(ratios.values()) <= dn.FACTOR, ratios


@pytest.mark.parametrize("name", LM_SCENES)
def test_scene_meets_its_conditions(name):
    a, b = scenes.literal(name, 0), scenes.literal(name, 1)
    assert a["iterations"] == b["iterations"] and a["trials"] == b["trials"] and a["decisions"] == b["decisions"]
    assert scenes.sequence(a["decisions"]) == scenes.expected_sequence(name)
    kw = scenes.run_kwargs(name)
    if name == "rejects":
        assert any(not ok for _, ok in a["decisions"])
    if name == "nbad":
        assert a["iterations"][0] < kw["n_iterations"] and a["trials"] == a["iterations"][0]
    if name == "robust_outliers":
        c = lit.bundle_adjustment(scenes.problem(name), order=0, deltas=lit.LOCAL_DELTAS, **kw)
        assert abs(c["chi2"][0] - a["chi2"][0]) > 1e-5 * a["chi2"][0]
    if name == "orphans":
        P = scenes.problem(name)
        assert (a["point_included"][-3:] == 0).all() and len(P["Tcw"]) - 1 not in set(np.asarray(P["edge_cam"]))
    if name == "stopped":
        assert a["iterations"] == (0, 0) and a["trials"] == 0
    if name == "stop_mid":
        assert a["trials"] == 3 and a["iterations"][0] < kw["n_iterations"]
    if name == "beyond_1024":
        P = scenes.problem(name)
        fixed = np.asarray(P["fixed"]).astype(bool)
        ec = np.asarray(P["edge_cam"])
        assert 6 * len(np.unique(ec[~fixed[ec]])) == 1032


def _spd(N):
    """test_gpu_reduced_system_ldlt's matrices."""
    rng = np.random.default_rng(N)
    M = rng.normal(size=(N, N))
    return np.ascontiguousarray(M @ M.T + 0.1 * N * np.eye(N)), rng.normal(size=N)


def _backward_error(S, b, x):
    return np.abs(S @ x - b).max() / (np.abs(S).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())


def tiled_ldlt_model(S, b, nb=64):
    """The tiled kernels' arithmetic in numpy: right-looking LDL^T without pivoting in nb-wide panels on the
    matrix padded with an identity block, entries kept unscaled (W = L D), b as an augmented row, then
    L^T x = D^-1 z from the last panel up in z's place.  None on an exactly zero pivot."""
    N = len(b)
    Np = (N + nb - 1) // nb * nb
    A = np.eye(Np + 1, Np)
    A[:N, :N] = S
    A[Np, :] = 0.0
    A[Np, :N] = b
    for j0 in range(0, Np, nb):
        T = A[j0:j0 + nb, j0:j0 + nb]
        for c in range(nb):
            d = T[c, c]
            if d == 0.0:
                return None
            l = T[c + 1:, c] * (1.0 / d)
            T[c + 1:, c + 1:] -= np.tril(np.outer(l, T[c + 1:, c]))
        dinv = 1.0 / np.diag(T)
        L11 = np.tril(T, -1) * dinv[None, :] + np.eye(nb)
        W = A[j0 + nb:, j0:j0 + nb]
        for m in range(nb - 1):
            W[:, m + 1:] -= np.outer(W[:, m], L11[m + 1:, m])
        A[j0 + nb:, j0 + nb:] -= W @ (W * dinv[None, :])[:Np - j0 - nb].T
    v = A[Np].copy()
    x = np.zeros(Np)
    for j0 in range(Np - nb, -1, -nb):
        T = A[j0:j0 + nb, j0:j0 + nb]
        for c in range(nb - 1, -1, -1):
            x[j0 + c] = v[j0 + c] * (1.0 / T[c, c])
            v[j0:j0 + c] -= T[c, :c] * x[j0 + c]
        v[:j0] -= A[j0:j0 + nb, :j0].T @ x[j0:j0 + nb]
    return x[:N]


@pytest.mark.parametrize("N", [6, 66, 258, 1032])
def test_tiled_ldlt_model_meets_the_criterion(N):
    """The bounds the GPU test holds the kernel to are the algorithm's: the model's error against numpy and
    its backward error relative to numpy's own."""
    S, b = _spd(N)
    x = tiled_ldlt_model(S, b)
    ref = np.linalg.solve(S, b)
    assert np.abs(x - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())
    assert _backward_error(S, b, x) <= 16 * _backward_error(S, b, ref)
    Z = np.eye(12)
    Z[5, 5] = 0.0
    assert tiled_ldlt_model(Z, np.ones(12)) is None


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ba(gpu):
    from orb_slam2_commit_amd import Optimizer
    o = Optimizer(0)
    yield o
    o.close()


def _run(ba, name, **dbg):
    kw = scenes.run_kwargs(name)
    after = kw.pop("raise_stop_after", -1)
    if after >= 0:
        dbg["raise_stop_after"] = after
    with ba.debug_options(**dbg):
        return ba.GlobalBundleAdjustemnt(scenes.problem(name), nIterations=kw["n_iterations"],
                                         stop=kw.get("stop", False), bRobust=kw["robust"])


def _compare_global(name, r):
    want = scenes.literal(name, 0)
    print(name, "gpu", r["iterations"], r["trials"], r["chi2"], "literal", want["iterations"], want["trials"],
          want["chi2"], "dT %.3g dX %.3g" % (np.abs(r["Tcw_d"] - want["Tcw_d"]).max(),
                                           np.abs(r["Xw_d"] - want["Xw_d"]).max() if len(r["Xw_d"]) else 0))
    _compare(r, want)
    assert r["ran"] == 1 and r["iterations"][1] == 0 and r["chi2"][1] == 0
    np.testing.assert_array_equal(r["point_included"], want["point_included"])
    P = scenes.problem(name)
    out = want["point_included"] == 0
    np.testing.assert_array_equal(r["Xw"][out], np.asarray(P["Xw"], np.float32)[out])  # returned unchanged


@pytest.mark.gpu
@pytest.mark.parametrize("name", LM_SCENES)
def test_gpu_globalba_matches_the_literal(ba, name):
    r = _run(ba, name)
    _compare_global(name, r)
    if name == "stopped":  # the inputs through toSE3Quat / toCvMat, exactly
        want = scenes.literal(name, 0)
        np.testing.assert_array_equal(r["Tcw"].view(np.uint32), want["Tcw"].view(np.uint32))
        np.testing.assert_array_equal(r["Xw"].view(np.uint32), want["Xw"].view(np.uint32))
        np.testing.assert_array_equal(r["Tcw_d"], want["Tcw_d"])
        np.testing.assert_array_equal(r["Xw_d"], want["Xw_d"])
    if name == "orphans":  # the keyframe without an edge keeps its pose (through the same conversions)
        np.testing.assert_array_equal(r["Tcw_d"][-1], scenes.literal(name, 0)["Tcw_d"][-1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["loop_small", "rejects", "mono_init"])
def test_gpu_globalba_tiled_kernel_forced(ba, name):
    """The tiled LDLT at sizes the single-workgroup kernels take by default: the same decisions, the same
    tolerance against the literal, identical bits from run to run."""
    a = _run(ba, name, ldlt=LDLT_TILED)
    _compare_global(name, a)
    b = _run(ba, name, ldlt=LDLT_TILED)
    for k in ("Tcw", "Xw", "Tcw_d", "Xw_d", "point_included"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["chi2"] == b["chi2"] and a["iterations"] == b["iterations"] and a["trials"] == b["trials"]
    d = _run(ba, name)
    assert d["iterations"] == a["iterations"] and d["trials"] == a["trials"]


def _ldlt(S, b, kind):
    from orb_slam2_commit_amd import _lib
    x = np.zeros(len(b))
    ms = C.c_float(0)
    rc = _lib.lib().orbx_debug_ldlt_ex(_lib.ptr(S), _lib.ptr(b), len(b), _lib.ptr(x), 1, C.byref(ms), kind, None)
    return rc, x


@pytest.mark.gpu
@pytest.mark.parametrize("N", [6, 66, 258, 1008, 1032, 3072])
def test_gpu_tiled_ldlt_solves(gpu, N):
    S, b = _spd(N)
    rc, x = _ldlt(S, b, LDLT_TILED)
    assert rc == 0
    ref = np.linalg.solve(S, b)
    err, be, be_ref = np.abs(x - ref).max(), _backward_error(S, b, x), _backward_error(S, b, ref)
    print("N %d: max|x - ref| %.3g, backward error %.3g (numpy's %.3g)" % (N, err, be, be_ref))
    assert err <= 1e-10 * max(1.0, np.abs(ref).max())
    assert be <= 16 * be_ref
    if N == 1008:  # the largest size the blocked kernel takes too
        rc2, x2 = _ldlt(S, b, 2)
        assert rc2 == 0 and np.abs(x - x2).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    if N == 1032:  # AUTO picks the tiled kernel there: the same bits
        rc0, x0 = _ldlt(S, b, 0)
        assert rc0 == 0 and np.array_equal(x0, x)


@pytest.mark.gpu
@pytest.mark.parametrize("N,k", [(12, 5), (258, 200)])
def test_gpu_tiled_ldlt_zero_pivot_fails_cleanly(gpu, N, k):
    from orb_slam2_commit_amd import _lib
    S = np.eye(N)
    S[k, k] = 0.0  # (N = 258, k = 200: a zero pivot in the fourth panel)
    rc, _ = _ldlt(S, np.ones(N), LDLT_TILED)
    assert rc == _lib.ORBX_ERR_STATE
    rc, x = _ldlt(np.eye(N), np.ones(N), LDLT_TILED)  # and the next solve is clean
    assert rc == 0 and np.array_equal(x, np.ones(N))


def _ceiling_problem(n_free):
    """n_free free keyframes + the fixed one, two points each, every point seen by its keyframe and the next."""
    nc = n_free + 1
    Tcw = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(1, 12), (nc, 1))
    Tcw[:, 3] = -0.01 * np.arange(nc)
    fixed = np.zeros(nc, np.uint8)
    fixed[0] = 1
    intr = np.tile(np.array([500, 500, 320, 240, 40], np.float32), (nc, 1))
    rng = np.random.default_rng(5)
    Xw = np.stack([rng.uniform(-2, 2, 2 * nc), rng.uniform(-1, 1, 2 * nc), rng.uniform(8, 12, 2 * nc)], 1).astype(np.float32)
    ep = np.repeat(np.arange(2 * nc), 2).astype(np.int32)
    ec = np.stack([np.arange(2 * nc) // 2, (np.arange(2 * nc) // 2 + 1) % nc], 1).reshape(-1).astype(np.int32)
    Pc = Xw[ep].astype(np.float64) + np.stack([Tcw[ec, 3], Tcw[ec, 7], Tcw[ec, 11]], 1)
    obs = np.stack([500 * Pc[:, 0] / Pc[:, 2] + 320, 500 * Pc[:, 1] / Pc[:, 2] + 240, -np.ones(len(ep))], 1)
    return dict(Tcw=Tcw, fixed=fixed, intr=intr, Xw=Xw, edge_point=ep, edge_cam=ec, obs=obs.astype(np.float32),
                inv_sigma2=np.ones(len(ep), np.float32))


@pytest.mark.gpu
def test_gpu_globalba_size_ceiling(ba):
    from orb_slam2_commit_amd import _lib
    with pytest.raises(_lib.OrbxError) as e:
        ba.GlobalBundleAdjustemnt(_ceiling_problem(513), nIterations=2, bRobust=False)
    assert e.value.code == _lib.ORBX_ERR_SIZE


@pytest.mark.gpu
def test_gpu_localba_untouched_by_a_global_call(ba):
    P = small_problem()
    a = ba.LocalBundleAdjustment(P)
    _run(ba, "loop_small")
    _run(ba, "robust_outliers")
    b = ba.LocalBundleAdjustment(P)
    for k in ("Tcw", "Xw", "Tcw_d", "Xw_d", "edge_outlier"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["iterations"] == b["iterations"] and a["trials"] == b["trials"] and a["chi2"] == b["chi2"]
    _compare(b, oracle.local_ba(P))
