"""Optimizer::BundleAdjustment (src/Optimizer.cc:49-284) restated in numpy float64, from the reference's text.

What is restated here, and calls nothing of liborbx:
  * the graph of :75-218 on a problem dict (cameras fixed where the caller says so, one edge per
    listed observation, ur < 0 monocular), Huber kernels only with bRobust, deltas thHuber2D =
    sqrt(5.99), thHuber3D = sqrt(7.815): double square roots stored in floats (:96-97), squared back
    into RobustKernelHuber's float _dsqr;
  * SparseOptimizer::optimize(n): the loop head polls terminate() before every iteration;
  * OptimizationAlgorithmLevenberg::solve: computeLambdaInit (tau = 1e-5 times the largest diagonal
    entry over pose and point blocks), scale = sum x (lambda x + b) + 1e-3, rho, lambda *= max(1/3,
    min(2/3, 1 - (2 rho - 1)^3)) and ni = 2 on success, lambda *= ni and ni *= 2 on failure (pop), at
    most 10 trials per iteration, stop on the exhausted budget or rho == 0, and this fork's _nBad
    rule (three iterations in a row that gain less than a thousandth of their starting chi2);
  * BlockSolver_6_3: H_pp, H_ll, H_pl, D = H_ll + lambda I, the Schur complement onto the free
    poses, the solve, the back substitution;
  * RobustKernelHuber (first-order weights rho') and activeRobustChi2;
  * the conversions around it: Converter::toSE3Quat (Eigen's matrix -> quaternion, normalised, w >= 0)
    on the way in, Converter::toCvMat(SE3Quat) (quaternion -> matrix, cast to float) on the way out.

The per-edge error and Jacobians come from oracle.ba_edge_probe and the pose update exp(x) * T from
oracle.se3_exp_mul, as in tests/localba_dense.py.

Every scene is run twice, with two assembly orders (edges forwards with numpy's inverse and solve,
edges backwards with the cofactor inverse): the difference is the restatement's own FP64 noise."""
import math

import numpy as np

import oracle

TH_HUBER_2D = float(np.float32(math.sqrt(5.99)))
TH_HUBER_3D = float(np.float32(math.sqrt(7.815)))
GLOBAL_DELTAS = (TH_HUBER_2D, TH_HUBER_3D)
# LocalBundleAdjustment's (src/Optimizer.cc:653-654: square roots of floats), for the scene conditions
LOCAL_DELTAS = (float(np.sqrt(np.float32(5.991))), float(np.sqrt(np.float32(7.815))))


# ---------------------------------------------------------------- conversions
def mat_to_quat(R):
    """Eigen::Quaterniond(Matrix3d) on a row-major 3x3 of Python floats -> (x, y, z, w)."""
    m = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
    t = m[0] + m[4] + m[8]
    if t > 0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return [(m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t, w]
    i = 0
    if m[4] > m[0]:
        i = 1
    if m[8] > (m[0] if i == 0 else m[4]):
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = math.sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0)
    q = [0.0, 0.0, 0.0, 0.0]
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (m[3 * k + j] - m[3 * j + k]) * t
    q[j] = (m[3 * j + i] + m[3 * i + j]) * t
    q[k] = (m[3 * k + i] + m[3 * i + k]) * t
    return q


def to_se3quat(Tcw):
    """Converter::toSE3Quat of one float 3x4 pose: SE3Quat(R, t) normalises its quaternion (w >= 0)."""
    T = np.asarray(Tcw, np.float32).astype(np.float64).reshape(3, 4)
    x, y, z, w = mat_to_quat(T[:, :3])
    if w < 0:
        x, y, z, w = -x, -y, -z, -w
    n = math.sqrt(x * x + y * y + z * z + w * w)
    return np.array([x / n, y / n, z / n, w / n]), T[:, 3].copy()


def quat_to_mat(q):
    """Eigen's Quaterniond::toRotationMatrix, row-major 3x3."""
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def to_cvmat(cq, ct):
    """Converter::toCvMat(SE3Quat) of every camera: [nc, 12] float64 (the caller casts to float)."""
    out = np.zeros((len(cq), 3, 4))
    for i in range(len(cq)):
        out[i, :, :3] = quat_to_mat(cq[i])
        out[i, :, 3] = ct[i]
    return out.reshape(len(cq), 12)


# ---------------------------------------------------------------- the graph
class Graph:
    def __init__(self, P, robust, deltas=GLOBAL_DELTAS):
        a = oracle.ba_arrays(P)
        self.a = a
        self.nc, self.np_, self.ne = len(a["Tcw"]), len(a["Xw"]), len(a["edge_point"])
        self.ec, self.ep = a["edge_cam"].astype(np.int64), a["edge_point"].astype(np.int64)
        self.obs = a["obs"].astype(np.float64)
        self.intr = a["intr"].astype(np.float64)
        self.info = a["inv_sigma2"].astype(np.float64)
        self.stereo = (a["obs"][:, 2] >= 0).astype(np.int64)
        self.robust = bool(robust)
        self.delta = np.where(self.stereo == 1, deltas[1], deltas[0])
        self.dsqr = np.float32(self.delta * self.delta).astype(np.float64)  # RobustKernelHuber's float _dsqr
        fixed = a["fixed"].astype(bool)
        cams = np.unique(self.ec)
        self.pose_cam = cams[~fixed[cams]]                 # free cameras with an edge, camera order
        self.pt_id = np.unique(self.ep)                    # points with an edge, point order
        self.cam_idx = -np.ones(self.nc, np.int64)
        self.cam_idx[self.pose_cam] = np.arange(len(self.pose_cam))
        self.pt_idx = -np.ones(self.np_, np.int64)
        self.pt_idx[self.pt_id] = np.arange(len(self.pt_id))
        self.ci, self.pi = self.cam_idx[self.ec], self.pt_idx[self.ep]
        self.point_included = np.zeros(self.np_, np.uint8)  # vbNotIncludedMP, :209-217
        self.point_included[self.pt_id] = 1
        qs, ts = zip(*(to_se3quat(T) for T in a["Tcw"])) if self.nc else ((), ())
        self.cq = np.array(qs, np.float64).reshape(self.nc, 4)
        self.ct = np.array(ts, np.float64).reshape(self.nc, 3)
        self.X = a["Xw"].astype(np.float64)
        # the same-point pairs (k1, k2) of edges on free cameras: the Schur complement's terms
        k1s, k2s = [], []
        free = np.where(self.ci >= 0)[0]
        order = np.argsort(self.ep[free], kind="stable")
        fe = free[order]
        starts = np.flatnonzero(np.r_[True, self.ep[fe][1:] != self.ep[fe][:-1], True])
        for s, e in zip(starts[:-1], starts[1:]):
            ks = fe[s:e]
            k1s.append(np.repeat(ks, len(ks)))
            k2s.append(np.tile(ks, len(ks)))
        self.k1 = np.concatenate(k1s) if k1s else np.zeros(0, np.int64)
        self.k2 = np.concatenate(k2s) if k2s else np.zeros(0, np.int64)
        self.free = free

    def edge_terms(self, jac=True):
        err, A, B = np.zeros((self.ne, 3)), np.zeros((self.ne, 3, 3)), np.zeros((self.ne, 3, 6))
        for e in range(self.ne):
            c, p = self.ec[e], self.ep[e]
            err[e], A[e], B[e] = oracle.ba_edge_probe(self.cq[c], self.ct[c], self.X[p], self.intr[c],
                                                      self.stereo[e], self.obs[e])
        return err, A, B

    def robust_chi2(self, err, reverse=False):
        """activeRobustChi2: rho(chi2) with a kernel, chi2 without."""
        c = self.info * (err ** 2).sum(axis=1)
        if self.robust:
            c = np.where(c <= self.dsqr, c, 2 * np.sqrt(c) * self.delta - self.dsqr)
        return float(np.sum(c[::-1]) if reverse else np.sum(c))

    def linearize(self, err, A, B, reverse=False):
        c = self.info * (err ** 2).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(c <= self.dsqr, 1.0, self.delta / np.sqrt(c)) if self.robust else np.ones(self.ne)
        W = self.info * w
        WA, WB = W[:, None, None] * A, W[:, None, None] * B
        Hll_e = np.einsum("kdr,kdc->krc", A, WA)
        bl_e = -np.einsum("kdr,kd->kr", WA, err)
        Hpp_e = np.einsum("kdr,kdc->krc", B, WB)
        bp_e = -np.einsum("kdr,kd->kr", WB, err)
        Hpl = np.einsum("kdr,kdc->krc", B, WA)
        npo, npt = len(self.pose_cam), len(self.pt_id)
        Hpp, bp = np.zeros((npo, 6, 6)), np.zeros((npo, 6))
        Hll, bl = np.zeros((npt, 3, 3)), np.zeros((npt, 3))
        od = np.arange(self.ne)[::-1] if reverse else np.arange(self.ne)
        np.add.at(Hll, self.pi[od], Hll_e[od])  # (unbuffered: the edges are added one by one, in od's order)
        np.add.at(bl, self.pi[od], bl_e[od])
        f = od[self.ci[od] >= 0]
        np.add.at(Hpp, self.ci[f], Hpp_e[f])
        np.add.at(bp, self.ci[f], bp_e[f])
        return dict(Hpp=Hpp, bp=bp, Hll=Hll, bl=bl, Hpl=Hpl)

    def lambda_init(self, L):
        m = 0.0
        if len(L["Hpp"]):
            m = max(m, float(np.abs(np.einsum("pii->pi", L["Hpp"])).max()))
        if len(L["Hll"]):
            m = max(m, float(np.abs(np.einsum("pii->pi", L["Hll"])).max()))
        return 1e-5 * m

    def reduced(self, L, lam, reverse=False):
        """(S, bs, Dinv): the Schur complement onto the free poses at damping lam."""
        npo, npt = len(self.pose_cam), len(self.pt_id)
        D = L["Hll"] + lam * np.eye(3)
        if reverse:  # cofactors
            m = D
            c = np.empty_like(m)
            c[:, 0, 0] = m[:, 1, 1] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 1]
            c[:, 0, 1] = m[:, 0, 2] * m[:, 2, 1] - m[:, 0, 1] * m[:, 2, 2]
            c[:, 0, 2] = m[:, 0, 1] * m[:, 1, 2] - m[:, 0, 2] * m[:, 1, 1]
            c[:, 1, 0] = m[:, 1, 2] * m[:, 2, 0] - m[:, 1, 0] * m[:, 2, 2]
            c[:, 1, 1] = m[:, 0, 0] * m[:, 2, 2] - m[:, 0, 2] * m[:, 2, 0]
            c[:, 1, 2] = m[:, 0, 2] * m[:, 1, 0] - m[:, 0, 0] * m[:, 1, 2]
            c[:, 2, 0] = m[:, 1, 0] * m[:, 2, 1] - m[:, 1, 1] * m[:, 2, 0]
            c[:, 2, 1] = m[:, 0, 1] * m[:, 2, 0] - m[:, 0, 0] * m[:, 2, 1]
            c[:, 2, 2] = m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 1, 0]
            det = m[:, 0, 0] * c[:, 0, 0] + m[:, 0, 1] * c[:, 1, 0] + m[:, 0, 2] * c[:, 2, 0]
            Dinv = c / det[:, None, None]
        else:
            Dinv = np.linalg.inv(D) if npt else np.zeros((0, 3, 3))
        S4 = np.zeros((npo, npo, 6, 6))
        idx = np.arange(npo)
        S4[idx, idx] = L["Hpp"] + lam * np.eye(6)
        bs = L["bp"].copy()
        k1, k2 = (self.k1[::-1], self.k2[::-1]) if reverse else (self.k1, self.k2)
        Y = L["Hpl"] @ Dinv[self.pi]                        # per edge: H_pl D^-1 (6 x 3)
        blk = np.einsum("krj,kcj->krc", Y[k1], L["Hpl"][k2])
        np.subtract.at(S4, (self.ci[k1], self.ci[k2]), blk)
        f = self.free[::-1] if reverse else self.free
        np.subtract.at(bs, self.ci[f], np.einsum("krj,kj->kr", Y[f], L["bl"][self.pi[f]]))
        N = 6 * npo
        return S4.transpose(0, 2, 1, 3).reshape(N, N), bs.reshape(N), Dinv

    def solve(self, L, lam, reverse=False):
        """BlockSolver::solve: (ok, xp[npo,6], xl[npt,3], S, bs)."""
        S, bs, Dinv = self.reduced(L, lam, reverse)
        npo = len(self.pose_cam)
        try:
            xp = np.linalg.solve(S, bs).reshape(npo, 6) if npo else np.zeros((0, 6))
        except np.linalg.LinAlgError:
            return False, None, None, S, bs
        if not np.isfinite(xp).all():
            return False, None, None, S, bs
        r = L["bl"].copy()
        f = self.free[::-1] if reverse else self.free
        np.subtract.at(r, self.pi[f], np.einsum("krj,kr->kj", L["Hpl"][f], xp[self.ci[f]]))
        xl = np.einsum("prc,pc->pr", Dinv, r)
        return True, xp, xl, S, bs

    def update(self, xp, xl):
        for i, c in enumerate(self.pose_cam):
            self.cq[c], self.ct[c] = oracle.se3_exp_mul(xp[i], self.cq[c], self.ct[c])
        self.X[self.pt_id] += xl


def first_step(P, robust, order=0):
    """The first trial's linear step (lambda from computeLambdaInit) at the input state: dict(S, bs, xp,
    xl, err, lam)."""
    G = Graph(P, robust)
    err, A, B = G.edge_terms()
    L = G.linearize(err, A, B, reverse=bool(order))
    lam = G.lambda_init(L)
    ok, xp, xl, S, bs = G.solve(L, lam, reverse=bool(order))
    assert ok
    return dict(S=S, bs=bs, xp=xp.reshape(-1), xl=xl, err=err, lam=lam, graph=G)


def bundle_adjustment(P, n_iterations, robust, stop=False, raise_stop_after=-1, order=0, deltas=GLOBAL_DELTAS):
    """BundleAdjustment on the problem dict.  stop: the flag is up before the call.  raise_stop_after =
    n >= 0: the flag reads raised at every poll after trial n (0-based) of the run, the rule of the
    library's debug hook.  order: 0 / 1, the two assembly orders.

    Returns LocalBundleAdjustment's result dict plus point_included, ran and decisions: one (iteration,
    accepted) pair per trial."""
    G = Graph(P, robust, deltas)
    rev = bool(order)
    trials, decisions = 0, []
    lam, ni, nBad = 0.0, 2.0, 0
    err = np.zeros((G.ne, 3))  # g2o's stored _error: zero until computeActiveErrors runs
    terminate = lambda: bool(stop) or (raise_stop_after >= 0 and trials > raise_stop_after)
    it = 0
    for i in range(int(n_iterations)):
        if terminate():
            break
        it += 1
        err, A, B = G.edge_terms()
        currentChi = G.robust_chi2(err, rev)
        iniChi = currentChi
        L = G.linearize(err, A, B, rev)
        if i == 0:
            lam, ni, nBad = G.lambda_init(L), 2.0, 0
        rho, qmax = 0.0, 0
        while True:
            bak = (G.cq.copy(), G.ct.copy(), G.X.copy())
            ok2, xp, xl, _, _ = G.solve(L, lam, rev)
            trials += 1
            if ok2:
                G.update(xp, xl)
            err = G.edge_terms()[0]
            tempChi = G.robust_chi2(err, rev)
            if not ok2:
                tempChi = float(np.finfo(np.float64).max)
            rho = currentChi - tempChi
            scale = 0.0
            if ok2:
                scale = float((xp * (lam * xp + L["bp"])).sum() + (xl * (lam * xl + L["bl"])).sum())
            scale += 1e-3
            rho /= scale
            accept = rho > 0 and math.isfinite(tempChi)
            if accept:
                alpha = 1.0 - (2 * rho - 1) ** 3
                alpha = min(alpha, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                currentChi = tempChi
            else:
                lam *= ni
                ni *= 2
                G.cq, G.ct, G.X = bak  # pop (the errors of the rejected estimate stay)
            decisions.append((i, bool(accept)))
            qmax += 1
            if not (rho < 0 and qmax < 10 and not terminate()):
                break
        if qmax == 10 or rho == 0:
            break
        if (iniChi - currentChi) * 1e3 < iniChi:
            nBad += 1
        else:
            nBad = 0
        if nBad >= 3:
            break
    chi = G.robust_chi2(err, rev)
    Tcw_d = to_cvmat(G.cq, G.ct)
    return dict(Tcw=Tcw_d.astype(np.float32), Xw=G.X.astype(np.float32), Tcw_d=Tcw_d, Xw_d=G.X.copy(),
                edge_outlier=np.zeros(G.ne, np.uint8), iterations=(it, 0), trials=trials, chi2=(chi, 0.0),
                point_included=G.point_included, ran=1, decisions=decisions)
