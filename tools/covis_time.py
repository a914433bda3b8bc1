"""Covisibility queries: the device-resident table (orbx_covis_*) against the reference's way, nested std::map
walks on the host (tools/covis_host.cpp, compiled next to this script).  Recorded, not gated; bench.py is the gate.

Workload: n keyframes of 1,000 features each along a path: keyframe i sees points 100 i .. 100 i + 999, so a
point is seen by ten consecutive keyframes and a keyframe shares points with nine on either side.  Octaves are
random in 0..3, three features in ten are stereo, all are close.  Per map size, median wall time per call over
the repeats, both sides called through ctypes with the same arrays:

  set_keyframe        the middle keyframe's row replaced by itself
  update_connections  of the middle keyframe, th = 15
  vote                with the middle keyframe's 1,000 points as the frame's
  local_points        of the 80 keyframes around the middle
  cull                the middle keyframe's 18 covisibles as candidates, monocular; the culled rows are put
                      back (untimed) before the next repeat

Both sides' results are compared (sizes of the counters, heads of the ordered lists, verdicts, local points).
Writes one JSON document (default profiles/covis_time.json) and prints it.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOST_SRC = os.path.join(ROOT, "tools", "covis_host.cpp")
HOST_LIB = os.path.join(ROOT, "tools", "micro", "libcovis_host.so")

FEATURES, STEP = 1000, 100


def host_lib():
    if not os.path.exists(HOST_LIB) or os.path.getmtime(HOST_LIB) < os.path.getmtime(HOST_SRC):
        os.makedirs(os.path.dirname(HOST_LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", HOST_LIB, HOST_SRC])
    L = C.CDLL(HOST_LIB)
    P = C.c_void_p
    L.covis_host_create.restype = P
    L.covis_host_destroy.argtypes = [P]
    L.covis_host_set_keyframe.argtypes = [P, C.c_int64, C.c_int, P, P, P]
    L.covis_host_update_connections.argtypes = [P, C.c_int64, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.covis_host_vote.argtypes = [P, P, C.c_int, C.POINTER(C.c_int64)]
    L.covis_host_local_points.argtypes = [P, P, C.c_int, P]
    L.covis_host_cull.argtypes = [P, P, C.c_int, P, C.c_int, P]
    return L


def make_map(rng, n_kf):
    rows = []
    for i in range(n_kf):
        pid = np.arange(STEP * i, STEP * i + FEATURES, dtype=np.int32)
        octv = rng.integers(0, 4, FEATURES).astype(np.int32)
        fl = (np.where(rng.random(FEATURES) < 0.3, 1, 0) | 2).astype(np.uint8)
        rows.append((pid, octv, fl))
    return rows


def median_ms(fn, repeats, warmup, after=None):
    ts = []
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        r = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if after:
            after(r)
        if k >= warmup:
            ts.append(dt)
    return round(statistics.median(ts), 4), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30,100,300,1000")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covis_time.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("covis_time needs the GPU: no number is taken without one")
    from orb_slam2_commit_amd import CovisibilityMap
    from orb_slam2_commit_amd._lib import ptr
    H = host_lib()
    out = dict(device=torch.cuda.get_device_name(0), features_per_keyframe=FEATURES, step=STEP, repeats=a.repeats,
               warmup=a.warmup, unit="ms, median wall time per call", sizes=[])
    rng = np.random.default_rng(1)
    for n_kf in [int(x) for x in a.sizes.split(",")]:
        rows = make_map(rng, n_kf)
        cm, hw = CovisibilityMap(0), H.covis_host_create()
        t0 = time.perf_counter()
        for i, r in enumerate(rows):
            cm.set_keyframe(i, *r)
        dev_build = time.perf_counter() - t0
        t0 = time.perf_counter()
        for i, r in enumerate(rows):
            H.covis_host_set_keyframe(hw, i, FEATURES, ptr(r[0]), ptr(r[1]), ptr(r[2]))
        host_build = time.perf_counter() - t0
        mid = n_kf // 2
        res = {}
        # set_keyframe
        d, _ = median_ms(lambda: cm.set_keyframe(mid, *rows[mid]), a.repeats, a.warmup)
        h, _ = median_ms(lambda: H.covis_host_set_keyframe(hw, mid, FEATURES, *[ptr(x) for x in rows[mid]]), a.repeats,
                         a.warmup)
        res["set_keyframe"] = dict(device=d, host=h)
        # update_connections
        d, (counter, ordered) = median_ms(lambda: cm.update_connections(mid, 15), a.repeats, a.warmup)
        no, first = C.c_int(), C.c_int64()
        h, nc = median_ms(lambda: H.covis_host_update_connections(hw, mid, 15, C.byref(no), C.byref(first)), a.repeats,
                          a.warmup)
        assert nc == len(counter) and no.value == len(ordered) and first.value == ordered[0][0], (nc, len(counter))
        res["update_connections"] = dict(device=d, host=h, counter=nc, ordered=no.value)
        # vote
        frame = rows[mid][0]
        d, (_, vc, kmax, _) = median_ms(lambda: cm.vote(frame), a.repeats, a.warmup)
        km = C.c_int64()
        h, nv = median_ms(lambda: H.covis_host_vote(hw, ptr(frame), len(frame), C.byref(km)), a.repeats, a.warmup)
        assert nv == len(vc) and km.value == kmax
        res["vote"] = dict(device=d, host=h, keyframes=nv)
        # local_points
        lk = np.arange(max(0, mid - 40), min(n_kf, mid + 40), dtype=np.int64)
        buf = np.zeros(len(lk) * FEATURES, np.int32)
        d, lp = median_ms(lambda: cm.local_points(lk, cap=len(buf)), a.repeats, a.warmup)
        h, nlp = median_ms(lambda: H.covis_host_local_points(hw, ptr(lk), len(lk), ptr(buf)), a.repeats, a.warmup)
        assert lp == buf[:nlp].tolist()
        res["local_points"] = dict(device=d, host=h, keyframes=len(lk), points=nlp)
        # cull: the covisibles of the middle keyframe in the graph's order, put back after every call
        cands = np.array([k for k, _ in ordered], np.int64)
        ne = np.zeros(len(cands), np.uint8)

        def restore_dev(r):
            for k, v in zip(cands, r[0]):
                if v == 1:
                    cm.set_keyframe(int(k), *rows[int(k)])

        hv = np.zeros(len(cands), np.uint8)

        def restore_host(_):
            for k, v in zip(cands, hv):
                if v == 1:
                    H.covis_host_set_keyframe(hw, int(k), FEATURES, *[ptr(x) for x in rows[int(k)]])

        d, (dv, dbad) = median_ms(lambda: cm.cull(cands, ne, True), a.repeats, a.warmup, restore_dev)
        h, _ = median_ms(lambda: H.covis_host_cull(hw, ptr(cands), len(cands), ptr(ne), 1, ptr(hv)), a.repeats,
                         a.warmup, restore_host)
        assert dv == hv.tolist() and dbad == [], (dv, hv.tolist())
        res["cull"] = dict(device=d, host=h, candidates=len(cands), culled=int(sum(v == 1 for v in dv)))
        live, pool, npts = cm.size()
        out["sizes"].append(dict(keyframes=n_kf, points=npts, build_device_s=round(dev_build, 3),
                                 build_host_s=round(host_build, 3), **res))
        cm.close()
        H.covis_host_destroy(hw)
    text = json.dumps(out, indent=1)
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
