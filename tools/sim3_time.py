"""Time the GPU Sim3Solver: one orbx_sim3_iterate_candidates sweep (5 candidates, N = 100,
iterate(5)) and find() with 300 hypotheses, beside orbx_pnp_iterate_candidates on the same launch
structure (5 candidates, N = 100, iterate(5)) and the literal restatement's single-thread Python time."""
import json
import sys
import time

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")

import numpy as np  # noqa: E402

from orb_slam2_commit_amd import PnPsolver, Sim3Solver, synth  # noqa: E402
from orb_slam2_commit_amd.glibc_rand import GlibcRand  # noqa: E402
from orb_slam2_commit_amd.orb import pnp_iterate_candidates, sim3_iterate_candidates  # noqa: E402

K = (520.9, 521.0, 325.1, 249.7)
LEVEL_SIGMA2 = [np.float32(1.2) ** (2 * l) for l in range(8)]


def problem(N, outliers, seed, noise=0.03):
    """N correspondences X1 = s R X2 + t with 3-D noise and a share of unrelated points."""
    g = np.random.RandomState(seed)
    X1 = np.stack([g.uniform(-2.5, 2.5, N), g.uniform(-1.8, 1.8, N), g.uniform(3.0, 9.0, N)], axis=1)
    a = g.normal(size=3)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.35) * Kx + (1 - np.cos(0.35)) * Kx @ Kx
    X2 = (X1 - np.array([0.4, -0.2, 0.3])) @ R / 1.3 + g.normal(size=(N, 3)) * noise
    out = g.permutation(N)[:int(round(outliers * N))]
    X2[out] = np.stack([g.uniform(-2.5, 2.5, len(out)), g.uniform(-1.8, 1.8, len(out)), g.uniform(3.0, 9.0, len(out))],
                       axis=1)
    return {"x3dc1": X1.astype(np.float32), "x3dc2": X2.astype(np.float32),
            "sigma2_1": np.array([LEVEL_SIGMA2[o] for o in g.randint(0, 8, N)], np.float32),
            "sigma2_2": np.array([LEVEL_SIGMA2[o] for o in g.randint(0, 8, N)], np.float32),
            "K1": K, "K2": K, "bFixScale": False}


def timed(fn, reps):
    fn()  # warm-up: first-use init, scratch growth
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def main(reps=50, literal=True):
    out = {}
    # every candidate far from a solution (all outliers), so each sweep runs all 5 x 5 hypotheses
    probs = [problem(100, 1.0, 40 + i) for i in range(5)]
    sols = Sim3Solver.create_many(probs, 0.99, 20, 300)

    def sweep():
        for s in sols:
            s.SetRansacParameters(0.99, 20, 300)   # mnIterations back to 0 (not timed separately: host only + 4 B memset)
        t0 = time.perf_counter()
        stopped, _ = sim3_iterate_candidates(sols, 5, GlibcRand(1))
        assert stopped == 5
        return time.perf_counter() - t0
    sweep()
    out["sim3_candidates_5x100_iterate5_ms"] = round(sum(sweep() for _ in range(reps)) / reps * 1e3, 4)

    big = Sim3Solver(**{k: probs[0][k] for k in ("x3dc1", "x3dc2", "sigma2_1", "sigma2_2", "K1", "K2", "bFixScale")})
    big.SetRansacParameters(0.99, 6, 300)

    def find():
        big.SetRansacParameters(0.99, 6, 300)
        t0 = time.perf_counter()
        T, _, _ = big.find(GlibcRand(1))
        assert T is None and big.mnIterations == 300
        return time.perf_counter() - t0
    find()
    out["sim3_find_300_hypotheses_N100_ms"] = round(sum(find() for _ in range(reps)) / reps * 1e3, 4)

    # the same launch structure on the PnP side, as a sanity reference
    pp = [synth.pnp_problem(seed=60 + i, n=100, outlier_frac=1.0, noise_px=0.5) for i in range(5)]

    def pnp_sweep():
        ps = PnPsolver.create_many(pp, 0.99, 10, 300, 4, 0.5, 5.991)
        t0 = time.perf_counter()
        pnp_iterate_candidates(ps, 5, GlibcRand(1))
        dt = time.perf_counter() - t0
        for p in ps:
            p.close()
        return dt
    pnp_sweep()
    out["pnp_candidates_5x100_iterate5_ms"] = round(sum(pnp_sweep() for _ in range(reps)) / reps * 1e3, 4)

    if literal:
        import sim3_literal as lit
        P = probs[0]
        L = lit.Sim3Solver(P["x3dc1"], P["x3dc2"], P["sigma2_1"], P["sigma2_2"], K, K, False)
        t0 = time.perf_counter()
        L.find(GlibcRand(1))
        out["literal_python_single_thread_find_300_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
