"""Time the RGB-D front end on the GPU and write profiles/rgbd_time.json.

  frame_rgbd     : median of 20 orbx_frame_rgbd calls after a warm-up (host images in, host vectors out):
                   a 640 x 480 3-channel image with 16-bit depth, 1,000 features, TUM fr1 calibration
  caller_path    : what a caller had before this entry point existed, per frame: grey conversion in
                   numpy, orbx_extract, orbx_undistort_keypoints, a numpy depth lookup
  cvt_gray       : k_cvt_gray's HIP-event time for a device-resident batch of 256 images of 640 x 480, 3
                   and 4 channels, and its GB/s against the (C + 1) * W * H bytes per image it must move
Wall times are time.perf_counter around the whole call; nothing here is a gate.

usage: python tools/rgbd_time.py [out.json]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (before liborbx.so is loaded)

import rgbd_literal as lit  # noqa: E402
from orb_slam2_commit_amd import ORBextractor, _lib, frame_rgbd  # noqa: E402
from orb_slam2_commit_amd.orb import undistort_keypoints  # noqa: E402

W, H, NF, WARM, REPS, BATCH = 640, 480, 1000, 5, 20, 256
K = np.array([[517.306408, 0, 318.643040], [0, 516.469215, 255.313989], [0, 0, 1]], np.float32)
DIST = lit.DIST_TUM1
BF = 40.0


def _median_ms(fn):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), p90_ms=float(np.percentile(t, 90)))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rgbd_time.json")
    colour = lit.colour_image(21, W, H, 3)
    depth = lit.base_depth_u16(W, H)
    fac = lit.FACTOR_5000
    ex = ORBextractor(NF, 1.2, 8, 20, 7)
    res = dict(shape=[W, H], nfeatures=NF, warmup=WARM, reps=REPS, device=torch.cuda.get_device_name(0))

    one = frame_rgbd(ex, colour, depth, fac, K, DIST, BF)
    res["keypoints"] = int(len(one[0]))
    res["frame_rgbd"] = _median_ms(lambda: frame_rgbd(ex, colour, depth, fac, K, DIST, BF))

    def caller_path():
        grey = lit.gray(colour, True)
        kps, desc = ex(grey)
        un = undistort_keypoints(kps, K, DIST)
        d = depth[kps["y"].astype(np.int64), kps["x"].astype(np.int64)].astype(np.float32) * fac
        ok = d > 0
        u_right = np.where(ok, un["x"] - np.float32(BF) / np.where(ok, d, np.float32(1)), np.float32(-1))
        return kps, desc, un, u_right, np.where(ok, d, np.float32(-1))

    two = caller_path()
    res["caller_path_equal"] = bool(all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(one, two)))
    res["caller_path"] = _median_ms(caller_path)
    res["caller_path"]["steps"] = "numpy grey conversion, orbx_extract, orbx_undistort_keypoints, numpy depth lookup"

    # k_cvt_gray alone on a device batch
    L = _lib.lib()
    dev = torch.device("cuda:0")
    res["cvt_gray"] = {}
    for ch in (3, 4):
        src = torch.randint(0, 256, (BATCH, H, W, ch), dtype=torch.uint8, device=dev)
        dst = torch.empty((BATCH, H, W), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream()

        def launch():
            _lib.check(L.orbx_cvt_gray_device(ex._h, _lib.ptr(src), W * ch, W * H * ch, BATCH, W, H, ch, 1, _lib.ptr(dst), W,
                                              W * H, C.c_void_p(1)), "orbx_cvt_gray_device")
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            launch()
            e1.record(st)
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        nbytes = (ch + 1) * W * H * BATCH
        res["cvt_gray"]["%d_channels" % ch] = dict(images=BATCH, event_ms_median=ms, event_ms_min=float(np.min(times)),
                                                   bytes=nbytes, gb_per_s=nbytes / ms / 1e6)
        k = 7
        assert np.array_equal(dst[k].cpu().numpy(), lit.gray(src[k].cpu().numpy(), True))
    res["not_measured"] = ("the shim's Frame constructor, orbx_rgbd_frames_device, counters (FETCH_SIZE / WRITE_SIZE) of "
                           "k_cvt_gray; the batch sits in the 256 MiB L3 only in part (%d MiB source)" % (BATCH * W * H * 3 >> 20))
    ex.close()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
