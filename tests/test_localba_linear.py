"""LocalBundleAdjustment's linear step, trial by trial, against a dense high-precision reference.

test_localba.py compares the GPU solver with the oracle at the end of a whole LM run, which is blind
to an error in the matrix side of a trial (H_pp, H_ll, H_pl, the Schur complement): the run converges
to the same poses anyway.  Here one chosen trial is captured (include/orbx_debug.h,
orbx_debug_ba_capture_*) and its structure, S, b_s, x_p, the point step and the stored errors are
compared with tests/localba_dense.py: a longdouble assembly of the same step, with the bound set at
16 times the noise two float64 assemblies of the reference itself show.  The CPU half holds the
oracle's Schur code to the same comparison and shows that the comparison rejects four seeded defects."""
import numpy as np
import pytest

import localba_dense as dn
import oracle
from test_localba import reject_problem, small_problem

CPU_CASES = ["tiny", "fuse_blocks", "deg34", "mono_only"]
GPU_CASES = ["tiny", "fuse_blocks", "shuffled", "deg34", "long_lists", "n126", "n132", "n192", "n198", "mono_only"]
SELECTORS = [(0, 0, 0), (0, 1, 0), (1, 0, 0)]
kFuseStride, kFuseMaxDeg, kUpCh, kUpPts = 96, 32, 2048, 64  # csrc/ba_linearize.h, ba_lm.h


def _inliers(T):
    th = np.where(T["stereo"] == 1, dn.TH_STEREO, dn.TH_MONO)
    return (dn.chi2(T) <= th) & (T["depth"] > 0)


def _lambda_init(P, T, act, robust):
    """computeLambdaInit: tau * max |H_jj| over the active vertices."""
    s = dn.assemble(P, T, act, robust, 1.0)
    d = [np.abs(np.einsum("pii->pi", s[k])).max() for k in ("Hpp", "Hll") if s[k].size]
    return 1e-5 * float(max(d))


# ---------------------------------------------------------------- CPU: the cases reach what they claim
def test_cases_reach_the_kernel_constants():
    deg = lambda P: np.bincount(np.asarray(P["edge_point"]), minlength=len(P["Xw"]))
    P = dn.problem("tiny")
    ep, ec = np.asarray(P["edge_point"]), np.asarray(P["edge_cam"])
    d = deg(P)
    assert (d == 1).any() and len(ep) < 64
    only_fixed = [p for p in np.unique(ep) if (ec[ep == p] == 2).all()]
    assert only_fixed and list(P["fixed"]) == [0, 0, 1]
    st = np.asarray(P["obs"])[:, 2] >= 0
    assert st.any() and (~st).any()
    P = dn.problem("fuse_blocks")
    assert (len(P["edge_point"]) - 1) // kFuseStride + 1 >= 12 and deg(P).max() <= kFuseMaxDeg
    assert (np.diff(P["edge_point"]) >= 0).all() and not (np.diff(dn.problem("shuffled")["edge_point"]) >= 0).all()
    P = dn.problem("deg34")
    d = deg(P)
    assert d.max() > kFuseMaxDeg and (np.diff(P["edge_point"]) >= 0).all()
    assert d[d > 0][:kUpPts].sum() > kUpCh and (d > 0).sum() >= kUpPts
    assert (~np.asarray(P["fixed"], bool)).sum() == 30  # N = 180
    P = dn.problem("long_lists")
    free = ~np.asarray(P["fixed"], bool)
    assert np.bincount(P["edge_cam"])[free].max() > 512
    assert not (np.asarray(dn.problem("mono_only")["obs"])[:, 2] >= 0).any()


# ---------------------------------------------------------------- CPU: oracle against the dense reference
@pytest.mark.parametrize("mode", ["robust_all", "inliers"])
@pytest.mark.parametrize("case", CPU_CASES)
def test_oracle_linear_step_matches_dense(case, mode):
    """oracle_ba_linear_step (the oracle's build_system + solve_damped) at the problem's initial state,
    on every edge with Huber (phase 1's form) and on the chi2 inliers without (phase 2's)."""
    P = dn.problem(case)
    ne = len(P["edge_point"])
    cq, ct, X = dn.initial_state(P)
    T = dn.edge_terms(P, cq, ct, X)
    if mode == "robust_all":
        active, robust = np.ones(ne, bool), np.ones(ne, np.uint8)
    else:
        active, robust = _inliers(T), np.zeros(ne, np.uint8)
        assert 0 < active.sum() < ne or case == "tiny"
    act = np.where(active)[0]
    lam = _lambda_init(P, T, act, robust)
    R = dn.Reference(P, T, act, robust, lam)
    o = oracle.ba_linear_step(P, cq, ct, X, active, robust, lam)
    assert o["ok"] and o["nposes"] == len(R.ld["pose_cam"]) and o["npts"] == len(R.ld["pt_id"])
    ratios = R.ratios(dict(S=o["S"], bs=o["bs"], xp=o["xp"], xl=o["xl"], eerr=o["err"][act]))
    dn.report("oracle %s %s" % (case, mode), ratios)
    for q in dn.QUANTITIES:
        assert ratios[q] <= dn.FACTOR, (q, ratios)


# ---------------------------------------------------------------- CPU: the comparison rejects seeded defects
@pytest.fixture(scope="module")
def fuse_ref():
    P = dn.problem("fuse_blocks")
    ne = len(P["edge_point"])
    cq, ct, X = dn.initial_state(P)
    T = dn.edge_terms(P, cq, ct, X)
    act, robust = np.arange(ne), np.ones(ne, np.uint8)
    lam = _lambda_init(P, T, act, robust)
    return dn.Reference(P, T, act, robust, lam)


@pytest.mark.parametrize("defect", ["pair", "hpp_last", "stale_lambda", "rho1"])
def test_comparison_rejects_seeded_defect(fuse_ref, defect):
    """A float64 system built by the reference's own code with one error seeded -- (a) one edge pair's
    term missing from one off-diagonal S block, (b) one pose's H_pp without its last position, (c) D^-1
    formed with the previous lambda (3 lambda: the step an accepted trial takes), (d) one robust edge
    weighted with rho' = 1 -- must exceed the 16x bound; the same system without the defect passes."""
    R = fuse_ref
    P, ld = R.P, R.ld
    ci, pi = ld["ci"], ld["pi"]
    if defect == "pair":
        k1 = next(k for k in range(len(ci)) if ci[k] >= 0 and ((pi == pi[k]) & (ci >= 0) & (ci != ci[k])).any())
        k2 = np.where((pi == pi[k1]) & (ci >= 0) & (ci != ci[k1]))[0][0]
        d = ("pair", k1, int(k2))
    elif defect == "hpp_last":
        d = ("hpp_last", 2)
    elif defect == "stale_lambda":
        d = ("stale_lambda", 3.0 * R.lam)
    else:
        w = dn.huber_weight(R.T)[R.act]
        d = ("rho1", int(np.where((w < 1.0) & (ci >= 0))[0][0]))
    clean = R.ratios(R.f64[0])
    bad = R.ratios(dn.assemble(P, R.T, R.act, R.robust, R.lam, np.float64, inverse="np", solve=True, defect=d))
    dn.report("defect %s" % defect, bad)
    assert max(clean.values()) <= 1.0  # (it is one of the two runs the noise is the maximum of)
    assert bad["S"] > dn.FACTOR, bad
    if defect in ("stale_lambda", "rho1"):
        assert bad["bs"] > dn.FACTOR and bad["xl"] > dn.FACTOR, bad
    # the broken system's own solution does not solve the reference system either
    assert bad["xp"] > dn.FACTOR, bad


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ba(gpu):
    from orb_slam2_commit_amd import Optimizer
    o = Optimizer(0)
    yield o
    o.close()


_baseline = {}


def _run_captured(ba, name, P, sel):
    """One run with the capture armed; asserts it is bit-identical to the run without (cached per problem)."""
    if name not in _baseline:
        _baseline[name] = ba.LocalBundleAdjustment(P)
    ba.capture_select(*sel)
    r = ba.LocalBundleAdjustment(P)
    c = ba.capture_read()
    b = _baseline[name]
    for k in ("Tcw", "Xw", "Tcw_d", "Xw_d", "edge_outlier"):
        np.testing.assert_array_equal(np.asarray(r[k]), np.asarray(b[k]))
    assert list(r["iterations"]) == list(b["iterations"]) and r["trials"] == b["trials"] and r["chi2"] == b["chi2"]
    return r, c


def _check_capture(tag, P, c, sel, check_active_set=False):
    """Everything a capture is held to; returns the GPU / noise ratios."""
    phase, it, q = sel
    ne = len(P["edge_point"])
    assert c["phase"] == phase and c["q"] == q and (it < 0 or c["it"] == it) and c["ok"] == 1
    assert (c["nc"], c["np"], c["ne"]) == (len(P["fixed"]), len(P["Xw"]), ne)
    if q == 0:  # nothing to pop: the errors were computed at the state the trial is linearised at
        for k in ("cq", "ct", "X"):
            np.testing.assert_array_equal(c[k], c[k + "_lin"])
    act = c["act"].astype(np.int64)
    ep = np.asarray(P["edge_point"])
    # ---- structure, exact
    assert len(np.unique(act)) == len(act) == c["na"]
    np.testing.assert_array_equal(act, np.sort(act)[np.argsort(ep[np.sort(act)], kind="stable")])  # point-major, stable
    pose_cam, pt_id = dn.structure(P, act)
    np.testing.assert_array_equal(c["pose_cam"], pose_cam)
    np.testing.assert_array_equal(c["pt_id"], pt_id)
    assert c["nposes"] == len(pose_cam) and c["npa"] == len(pt_id)
    robust = c["erobust"]
    T_all = None
    if phase == 0:
        np.testing.assert_array_equal(np.sort(act), np.arange(ne))
        assert (robust == 1).all()
    else:
        assert (robust == 0).all()
        if check_active_set:
            T_all = dn.edge_terms(P, c["cq"], c["ct"], c["X"])
            np.testing.assert_array_equal(np.sort(act), np.where(_inliers(T_all))[0])
    # ---- the linear step
    T = T_all if (T_all is not None and q == 0) else dn.edge_terms(P, c["cq_lin"], c["ct_lin"], c["X_lin"], act)
    R = dn.Reference(P, T, act, robust, c["lambda"], Xbak=c["Xbak"])
    ratios = R.ratios(dict(S=c["S"], bs=c["bs"], xp=c["xp"], xl=c["xl"], eerr=c["eerr"][act]))
    if q > 0:  # a retry: the stored errors are the rejected estimate's (the current state's)
        Tc = dn.edge_terms(P, c["cq"], c["ct"], c["X"], act)
        ratios["eerr"] = dn.dev(c["eerr"][act], Tc["err"][act]) / dn.FLOOR
    chi = dn.robust_chi(T, act, robust)
    assert abs(np.longdouble(c["chi"]) - chi) <= 1e-12 * abs(chi), (c["chi"], float(chi))
    dn.report(tag, ratios)
    for k in dn.QUANTITIES:
        assert ratios[k] <= dn.FACTOR, (k, ratios)
    return ratios


@pytest.mark.gpu
@pytest.mark.parametrize("sel", SELECTORS, ids=lambda s: "p%d_it%d_q%d" % s)
@pytest.mark.parametrize("case", GPU_CASES)
def test_gpu_linear_step_matches_dense(ba, case, sel):
    """GPU / noise per case, selector and quantity: the table in DESIGN.md (LocalBA test section)."""
    P = dn.problem(case)
    r, c = _run_captured(ba, case, P, sel)
    assert c is not None, "the selected trial did not run: %r" % (r["iterations"],)
    if case in dn.NPOSES_CASES:
        assert c["nposes"] == dn.NPOSES_CASES[case]  # the LDLT kernel this case is there for
    o = oracle.local_ba(P)
    _check_capture("%s %s" % (case, sel), P, c, sel, check_active_set=o["trials"] == sum(o["iterations"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small4", "nbad_stop"])
def test_gpu_phase2_active_set(ba, name):
    """Phase 2's active set is {e : chi2_ref(e) <= 5.991 / 7.815 and depth > 0} at the captured state, on
    the two problems known to run without a rejected trial (after one, g2o classifies with the
    rejected estimate's errors)."""
    P = small_problem(seed=4) if name == "small4" else reject_problem(name)
    o = oracle.local_ba(P)
    assert o["trials"] == sum(o["iterations"])
    r, c = _run_captured(ba, name, P, (1, 0, 0))
    assert c is not None
    _check_capture("%s (1, 0, 0)" % name, P, c, (1, 0, 0), check_active_set=True)


@pytest.mark.gpu
def test_gpu_retry_trial_matches_dense(ba):
    """The first retry of each phase of rejects_b (no relinearisation, a new lambda, the previous trial
    popped inside k_ba_update): the same comparison, and the retry steps from the state its
    iteration's first trial was linearised at."""
    P = reject_problem("rejects_b")
    fired = 0
    for phase in (0, 1):
        sel = (phase, -1, 1)
        r, c = _run_captured(ba, "rejects_b", P, sel)
        if c is None:
            continue
        fired += 1
        _check_capture("rejects_b %s" % (sel,), P, c, sel)
        r0, c0 = _run_captured(ba, "rejects_b", P, (phase, c["it"], 0))
        assert c0 is not None and c0["trial"] == c["trial"] - 1
        for k in ("cq_lin", "ct_lin", "X_lin"):
            np.testing.assert_array_equal(c[k], c0[k])
        assert c["lambda"] > c0["lambda"]  # a rejection raises lambda
        assert c["chi"] == c0["chi"]        # and leaves the iteration's chi
        assert np.abs(c["X"] - c["X_lin"]).max() > 0  # the rejected estimate was still in place
        assert np.abs(c["X"][c0["pt_id"]] - (c0["Xbak"] + c0["xl"])).max() <= 4 * 2.0 ** -52 * np.abs(c["X"]).max()
        _check_capture("rejects_b %s" % ((phase, c["it"], 0),), P, c0, (phase, c["it"], 0))
    assert fired >= 1


@pytest.mark.gpu
def test_gpu_capture_off_and_unfired(ba):
    """No capture without a selection; a selection holds for one run; a trial that never runs reports
    not fired and leaves the result alone."""
    P = dn.problem("tiny")
    ba.capture_select(-1)
    ba.LocalBundleAdjustment(P)
    assert ba.capture_read() is None
    r, c = _run_captured(ba, "tiny", P, (0, 0, 0))
    assert c is not None
    ba.LocalBundleAdjustment(P)  # the selection was consumed; the last capture stays readable
    c2 = ba.capture_read()
    assert c2 is not None and c2["trial"] == 0
    r, c = _run_captured(ba, "tiny", P, (0, 7, 0))  # optimize(5) has no iteration 7
    assert c is None
