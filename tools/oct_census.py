"""Per-level FAST survivor counts (k_octree's T) on bench-like KITTI frames, beside the LDS slots
the plan gives k_octree (its launch group's OctGroup::kcap): candidates past kcap live in global scratch and are
re-read every split round on the generic path.  Then, per level, how many blocks of the batch took each
path (0 empty level, 1 count pyramid, 2 generic): the frames' own candidates (ORBX_DBG_CELL_COUNTS,
ORBX_DBG_CANDIDATES) go back through orbx_debug_octree_paths as one batch, which runs the launch groups as
the benchmark's batches do.   usage: python tools/oct_census.py [stereo frames, default 8]"""
import json
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from orb_slam2_commit_amd import ORBextractor, _lib, synth  # noqa: E402
from orb_slam2_commit_amd.orb import debug_launch_plan, debug_octree_paths  # noqa: E402


def dbg(ex, what, image=0, arg=0, dtype=np.int32):
    L = _lib.lib()
    n = L.orbx_debug_copy(ex._h, what, image, arg, None, 0)
    buf = np.zeros(n, np.uint8)
    L.orbx_debug_copy(ex._h, what, image, arg, _lib.ptr(buf), n)
    return buf.view(dtype)


def main(n=8):
    imgs = synth.stereo_batch(0, n)
    ex = ORBextractor(2000, 1.2, 8, 20, 7)
    per, all_counts, all_cand = [], [], []
    for i in range(2 * n):
        ex(imgs[i])
        cells = dbg(ex, 3).reshape(-1, 8)
        counts = dbg(ex, 2)
        T = np.bincount(cells[:, 0], weights=counts, minlength=8).astype(int)
        ncell = np.bincount(cells[:, 0], minlength=8)
        per.append(T)
        all_counts.append(counts.copy())
        all_cand.append(dbg(ex, 4, dtype=np.uint32).copy())
    per = np.array(per)
    print(json.dumps(dict(T_mean=per.mean(0).round(1).tolist(), T_max=per.max(0).tolist(),
                          cells_per_level=ncell.tolist())))
    h, w = imgs[0].shape
    rows = debug_launch_plan(ex.params, w, h, 13).reshape(-1, 8)  # ORBX_LP_OCT_PYRAMID
    paths = np.concatenate([debug_octree_paths(ex, np.stack(all_counts[i:i + 32]), np.stack(all_cand[i:i + 32]))[2]
                            for i in range(0, 2 * n, 32)])
    census = {"level %d" % l: {"empty": int((paths[:, l] == 0).sum()), "pyramid": int((paths[:, l] == 1).sum()),
                               "generic": int((paths[:, l] == 2).sum())} for l in range(paths.shape[1])}
    print(json.dumps(dict(images=2 * n, pyramid_depth_per_row=rows[:, 0].tolist(), paths=census,
                          generic_blocks=int((paths == 2).sum()), blocks=int(paths.size))))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8)
