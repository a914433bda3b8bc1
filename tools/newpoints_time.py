"""Time LocalMapping::CreateNewMapPoints on the GPU (one MI355X).

  * one orbx_create_new_map_points at 10 stereo and at 20 monocular neighbours of 2,000 features each, host
    call to host result, the median of 20 calls after a warm-up call on the same handle;
  * beside it the only path the library had for the same matches before: that many
    orbx_search_for_triangulation host calls (the gates, F12 and the triangulation itself had no GPU form;
    F12 is computed here in float64 and not timed);
  * the device form between two stream events, and the same neighbours' searches alone
    (orbx_search_for_triangulation_device, one call per neighbour) between two events.  The second is not a
    share of the first: unchained, every search sees all of the current keyframe's features, and every call
    takes a stream-ordered block of its own.  The search's share of the chain is not measured here.
Writes profiles/newpoints_time.json (or the path given) and prints it.  No number here is a gate."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
from orb_slam2_commit_amd import LocalMapping, ORBmatcher, _lib, synth  # noqa: E402
from orb_slam2_commit_amd.orb import new_points_problem, tri_problem  # noqa: E402

REPS = 20


def search_problems(P):
    """The orbx_tri_problem dicts a caller of the search alone builds (F12 in float64)."""
    K1 = P["current"]
    T1 = np.asarray(K1["Tcw"], np.float64)
    Km = lambda K: np.array([[K["fx"], 0, K["cx"]], [0, K["fy"], K["cy"]], [0, 0, 1]], np.float64)  # noqa: E731
    out = []
    for K2 in P["neighbours"]:
        T2 = np.asarray(K2["Tcw"], np.float64)
        R12 = T1[:3, :3] @ T2[:3, :3].T
        t12 = -R12 @ T2[:3, 3] + T1[:3, 3]
        tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
        F12 = np.linalg.inv(Km(K1)).T @ tx @ R12 @ np.linalg.inv(Km(K2))
        side = lambda K: {k: K[k] for k in ("keys_un", "desc", "u_right", "has_mp", "node_id", "node_off", "feat")}  # noqa: E731
        out.append(dict(kf1=side(K1), kf2=side(K2), F12=F12.astype(np.float32),
                        C1w=(-T1[:3, :3].T @ T1[:3, 3]).astype(np.float32), T2w=T2.astype(np.float32), fx=K2["fx"],
                        fy=K2["fy"], cx=K2["cx"], cy=K2["cy"], scale_factors2=K2["scale_factors"],
                        level_sigma2_2=K2["level_sigma2"]))
    return out


def to_device(K, dev):
    import torch
    out = dict(K)
    for k in ("keys_un", "desc", "u_right", "has_mp", "node_id", "node_off", "feat", "keys_xy", "depth", "mp_pos"):
        a = np.ascontiguousarray(K[k])
        if k == "node_id":
            a = a.view(np.int32)
        out[k] = torch.from_numpy(a.view(np.uint8) if k == "keys_un" else a).to(dev)
    return out


def median_ms(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def device_ms(fn, reps=REPS):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def case(monocular, nn):
    import torch
    dev = torch.device("cuda:0")
    P = synth.new_points_problem(21, nn, n=2000, n_scene=1200, monocular=monocular)
    lm = LocalMapping(monocular, 0)
    r = lm.CreateNewMapPoints(P)
    call = median_ms(lambda: lm.CreateNewMapPoints(P))
    matcher = ORBmatcher(0.6, False)
    probs = search_problems(P)
    searches = median_ms(lambda: [matcher.SearchForTriangulation(pr) for pr in probs])
    # device forms between events
    n1 = len(P["current"]["desc"])
    Pd = dict(P, current=to_device(P["current"], dev), neighbours=[to_device(K, dev) for K in P["neighbours"]])
    p, keep = new_points_problem(Pd)
    out = dict(n_new=torch.zeros(1, dtype=torch.int32, device=dev),
               neighbours_done=torch.zeros(1, dtype=torch.int32, device=dev),
               point_idx=torch.zeros(3 * n1, dtype=torch.int32, device=dev),
               point_pos=torch.zeros(3 * n1, device=dev), point_normal=torch.zeros(3 * n1, device=dev),
               point_dist=torch.zeros(2 * n1, device=dev), nb_skip=torch.zeros(nn, dtype=torch.int32, device=dev),
               nb_nmatches=torch.zeros(nn, dtype=torch.int32, device=dev), nb_baseline=torch.zeros(nn, device=dev),
               nb_median_depth=torch.zeros(nn, device=dev), has_mp1=torch.zeros(n1, dtype=torch.uint8, device=dev))
    res = _lib.NewPointsResult()
    for k, v in out.items():
        setattr(res, k, v.data_ptr())
    has0 = Pd["current"]["has_mp"]
    s = torch.cuda.current_stream()
    L = _lib.lib()

    def chain():
        out["has_mp1"].copy_(has0)
        _lib.check(L.orbx_create_new_map_points_device(lm._h, C.byref(p), C.byref(res), C.c_void_p(s.cuda_stream)),
                   "device")

    chain_ms = device_ms(chain)
    tri, hold = [], []
    for pr in probs:
        d = dict(pr, kf1={k: Pd["current"][k] for k in pr["kf1"]}, kf2=None)
        K2 = Pd["neighbours"][len(tri)]
        d["kf2"] = {k: K2[k] for k in pr["kf2"]}
        t, kp = tri_problem(d, False, False)
        m, nm = torch.zeros(n1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        t.match12, t.nmatches = m.data_ptr(), nm.data_ptr()
        tri.append((_lib.TriProblem * 1)(t))
        hold.append((d, kp, m, nm))

    def search_only():
        out["has_mp1"].copy_(has0)
        for a in tri:
            _lib.check(L.orbx_search_for_triangulation_device(a, 1, C.c_void_p(s.cuda_stream)), "search")

    search_ms = device_ms(search_only)
    lm.close()
    return dict(monocular=bool(monocular), neighbours=nn, features=2000, n_new=int(r["n_new"]),
                matches=[int(x) for x in r["nb_nmatches"]], skipped=int((r["nb_skip"] != 0).sum()),
                create_new_map_points_ms=call, search_host_calls_ms=searches, chain_device_ms=chain_ms,
                unchained_searches_device_ms=search_ms, reps=REPS)


def main(out):
    res = dict(cases=[case(False, 10), case(True, 20)])
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "newpoints_time.json"))
