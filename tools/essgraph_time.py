"""Time the GPU Optimizer::OptimizeEssentialGraph on synthetic rings of 150, 500 and 1,500 keyframes.

The rings are tests/essgraph_scenes.py's (drifted odometry, a loop correction at the last keyframes) with
the covisibility graph widened to the reference's usual proportions: besides the spanning-tree edge each
keyframe has covisibility edges to the keyframes 2, 3 and 4 before it (weights >= 100), so about four
edges per keyframe, plus the old loop edge and the LoopConnections edges; 60 map points per keyframe.

Per size: ms per call (host pointers, scratch lease; a host clock around the synchronous call, mean after a
warm-up call), the Levenberg kernel's own phase times from orbx_debug_essgraph_phases (its 100 MHz wall
clock, summed over the run) divided per LM trial into linearise (per iteration: the 29 Sim3 logs per edge
and the assembly) / solve (envelope LDL^T and the substitutions) / update (oplus, errors, chi2, control),
the LM iteration and trial counts, and the envelope's block count.  The only CPU figure available is the
literal restatement's single-thread Python time at 150 keyframes -- not the reference's g2o speed.
Writes the JSON line to profiles/essgraph_time.json (or the path given) and prints it."""
import ctypes as C
import json
import sys
import time

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")

import numpy as np  # noqa: E402

from orb_slam2_commit_amd import _lib  # noqa: E402
from orb_slam2_commit_amd.orb import essential_graph_problem, essential_graph_structs  # noqa: E402


def ring(n, fix_scale, seed):
    import essgraph_scenes as scenes
    M = scenes.make_scene(n, fix_scale, seed, n_points=60 * n)
    bad = {kf["id"] for kf in M["keyframes"] if kf["bad"]}
    for kf in M["keyframes"]:
        cov = dict(kf["covisibles"])
        for d, w in ((3, 120), (4, 110)):
            for j in (kf["id"] - d, kf["id"] + d):
                if 0 <= j < len(M["keyframes"]) and j not in bad and j != kf["id"]:
                    cov[j] = max(cov.get(j, 0), w)
        kf["covisibles"] = sorted(cov.items(), key=lambda kv: (-kv[1], kv[0]))
    return M


def main(path=None, sizes=(150, 500, 1500), literal_at=150):
    import torch
    assert torch.cuda.is_available(), "no GPU: nothing here can be measured without one"
    torch.cuda.init()
    L = _lib.lib()
    out = {"sizes": list(sizes)}
    for n in sizes:
        M = ring(n, False, 9000 + n)
        P, ids, pts, edges = essential_graph_problem(M)
        p, r, o = essential_graph_structs(P)
        ms3 = np.zeros(3)
        blocks = C.c_longlong(0)

        def call():
            _lib.check(L.orbx_debug_essgraph_phases(C.byref(p), C.byref(r), _lib.ptr(ms3), C.byref(blocks), 0), "phases")
        call()  # warm-up: first-use init, scratch growth
        reps = 5 if n <= 500 else 2
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        ms = (time.perf_counter() - t0) / reps * 1e3
        its, trials = int(o["iterations"][0]), int(o["trials"][0])
        key = "n%d" % n
        out[key] = {"vertices": len(ids), "edges": len(edges), "points": len(pts), "unknowns": 7 * (len(ids) - 1),
                    "envelope_blocks": int(blocks.value), "call_ms": round(ms, 3), "lm_iterations": its,
                    "lm_trials": trials, "chi2": [float(o["chi2_initial"][0]), float(o["chi2_final"][0])],
                    "linearise_ms_per_iteration": round(float(ms3[0]) / max(its, 1), 3),
                    "solve_ms_per_trial": round(float(ms3[1]) / max(trials, 1), 3),
                    "update_ms_per_trial": round(float(ms3[2]) / max(trials, 1), 3),
                    "kernel_phase_ms_total": [round(float(v), 3) for v in ms3]}
        if n == literal_at:
            import essgraph_literal as lit
            t0 = time.perf_counter()
            ref = lit.run_problem(P)
            out[key]["literal_python_single_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            out[key]["equals_literal_bits"] = bool(
                np.array_equal(o["Scw_out"].view(np.uint64), ref["Scw_out"].view(np.uint64))
                and np.array_equal(o["Xw_out"].view(np.uint32), ref["Xw_out"].view(np.uint32))
                and its == ref["iterations"] and trials == ref["trials"])
    line = json.dumps(out)
    with open(path or ROOT + "/profiles/essgraph_time.json", "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main(*sys.argv[1:2])
