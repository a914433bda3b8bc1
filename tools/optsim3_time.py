"""Time the GPU Optimizer::OptimizeSim3: per-call latency of orbx_optimize_sim3 at n = 100
correspondences (host pointers, scratch lease) and the throughput of one orbx_optimize_sim3_device
launch of 256 problems, beside orbx_pose_optimization at 200 edges -- the nearest existing kernel
(the same Levenberg loop with an analytic Jacobian, so the difference is what the numeric
differentiation and the 7x7 solve cost) -- and the literal restatement's single-thread Python time.
Host calls: mean of 500 after a warm-up; device launches: HIP events around 200 back-to-back
launches on one stream.
Writes the JSON line to profiles/optsim3_time.json (or the path given) and prints it."""
import ctypes as C
import json
import sys
import time

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")

import numpy as np  # noqa: E402

from orb_slam2_commit_amd import Optimizer, _lib, synth  # noqa: E402
from orb_slam2_commit_amd.orb import optimize_sim3_problem_struct, pose_problem_struct  # noqa: E402


def timed(fn, reps):
    fn()  # warm-up: first-use init, scratch growth
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def main(path=None, reps=500, batch=256, launches=200):
    import torch
    import optsim3_literal as lit
    import optsim3_scenes as scenes
    dev = torch.device("cuda:0")
    torch.cuda.init()
    L = _lib.lib()
    out = {}
    P = scenes.make_problem(100, 0.3, 0, 7100)
    ref = lit.optimize_sim3(P)
    opt = Optimizer(0)
    got = opt.OptimizeSim3(P)
    assert got[0] == ref["n_in"] and np.array_equal(got[1].view(np.uint64), ref["S12"].view(np.uint64))
    out["optimize_sim3_n100_call_ms"] = round(timed(lambda: opt.OptimizeSim3(P), reps), 4)
    out["optimize_sim3_n100_lm_iterations"] = [int(v) for v in got[4]]
    out["optimize_sim3_n100_trials"] = int(got[5])

    pose = synth.pose_problem(900, n=200)
    out["pose_optimization_200_edges_call_ms"] = round(timed(lambda: opt.PoseOptimization(pose), reps), 4)
    out["pose_optimization_200_edges_lm_iterations"] = [int(v) for v in opt.PoseOptimization(pose)[3]]

    s = torch.cuda.current_stream()
    sp = C.c_void_p(s.cuda_stream)

    def device_ms(launch):
        launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(launches):
            launch()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches

    base = [scenes.make_problem(100, 0.3, b % 2, 7200 + b) for b in range(16)]
    probs, keep = [], []
    for b in range(batch):
        pr = base[b % 16]
        d = dict(pr)
        for k in ("x3dc1", "x3dc2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
            d[k] = torch.from_numpy(np.ascontiguousarray(pr[k], np.float32)).to(dev)
        outs = dict(S12_out=torch.zeros(8, dtype=torch.float64, device=dev),
                    inlier=torch.zeros(100, dtype=torch.uint8, device=dev),
                    n_in=torch.zeros(1, dtype=torch.int32, device=dev), n_bad=torch.zeros(1, dtype=torch.int32, device=dev),
                    iterations=torch.zeros(2, dtype=torch.int32, device=dev),
                    trials=torch.zeros(1, dtype=torch.int32, device=dev))
        probs.append(optimize_sim3_problem_struct(d, outs)[0])
        keep.append((d, outs))
    arr = (_lib.OptSim3Problem * batch)(*probs)
    ms = device_ms(lambda: _lib.check(L.orbx_optimize_sim3_device(arr, batch, sp), "orbx_optimize_sim3_device"))
    out["optimize_sim3_batch%d_n100_ms" % batch] = round(ms, 4)
    out["optimize_sim3_batch%d_problems_per_s" % batch] = round(batch / ms * 1e3, 1)

    pbase = [synth.pose_problem(900 + b, n=200) for b in range(16)]
    pprobs, pkeep = [], []
    for b in range(batch):
        pr = pbase[b % 16]
        d = {k: (torch.from_numpy(np.ascontiguousarray(pr[k])).to(dev) if k in ("obs", "Xw", "inv_sigma2") else pr[k])
             for k in pr}
        outs = dict(Tcw_out=torch.zeros(16, dtype=torch.float32, device=dev),
                    outlier=torch.zeros(200, dtype=torch.uint8, device=dev),
                    ngood=torch.zeros(1, dtype=torch.int32, device=dev),
                    iterations=torch.zeros(4, dtype=torch.int32, device=dev))
        pprobs.append(pose_problem_struct(d, outs)[0])
        pkeep.append((d, outs))
    parr = (_lib.PoseProblem * batch)(*pprobs)
    ms = device_ms(lambda: _lib.check(L.orbx_pose_optimization_device(parr, batch, sp), "orbx_pose_optimization_device"))
    out["pose_optimization_batch%d_200_edges_ms" % batch] = round(ms, 4)
    out["pose_optimization_batch%d_frames_per_s" % batch] = round(batch / ms * 1e3, 1)

    t0 = time.perf_counter()
    lit.optimize_sim3(P)
    out["literal_python_single_thread_n100_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    opt.close()
    line = json.dumps(out)
    with open(path or ROOT + "/profiles/optsim3_time.json", "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main(*sys.argv[1:2])
