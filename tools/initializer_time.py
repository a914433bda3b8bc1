"""Time the GPU Initializer: one Initialize call, host call to host result (mean of 50 after warm-up), at
N = 100, 300 and 1000 matches with 200 iterations, beside the literal restatement's single-thread Python
time for the same call.  Writes profiles/initializer_time.json.  There is no pass bar on these numbers:
the parent has no such call and the reference cannot be built here; they are recorded as what they are.

    python tools/initializer_time.py            # the timing, written to profiles/initializer_time.json
    python tools/initializer_time.py --calls 5  # a short run for a kernel trace (nothing written):
    rocprofv3 --kernel-trace --stats -- python tools/initializer_time.py --calls 5
"""
import json
import sys
import time

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before liborbx.so is loaded)

import initializer_scenes as S  # noqa: E402
from orb_slam2_commit_amd import orb  # noqa: E402
from orb_slam2_commit_amd.glibc_rand import GlibcRand  # noqa: E402


def main(reps=50, write=True):
    out = {"iterations": 200, "reps": reps}
    rv = np.array(GlibcRand(0).take(8 * 200), np.int32)
    for N in (100, 300, 1000):
        # a general scene with 10 % outliers and half as many unmatched keypoints again in each frame
        sc = S.make_scene("general", N, 900 + N, N // 2, N // 2 + 7, 0.1, 0.3)
        I = orb.Initializer(sc["keys1"], sc["K"], 1.0, 200)
        first = time.perf_counter()
        I.initialize_values(sc["keys2"], sc["matches12"], rv)
        first = time.perf_counter() - first
        I.initialize_values(sc["keys2"], sc["matches12"], rv)
        t0 = time.perf_counter()
        for _ in range(reps):
            ok = I.initialize_values(sc["keys2"], sc["matches12"], rv)[2]
        dt = (time.perf_counter() - t0) / reps
        key = "initialize_N%d_it200" % N
        out[key + "_call_ms"] = round(dt * 1e3, 4)
        out[key + "_first_call_ms"] = round(first * 1e3, 3)
        out[key + "_ok"] = bool(ok)
        out[key + "_model"] = "HF"[I.result["model"]]
        if write:
            t0 = time.perf_counter()
            lit_out, rec, _ = S.run_literal(sc, 200)
            out[key + "_literal_python_single_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert bool(lit_out[0]) == bool(ok) and rec["SF"] == I.result["SF"]
        I.close()
    print(json.dumps(out))
    if write:
        with open(ROOT + "/profiles/initializer_time.json", "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    if "--calls" in sys.argv:
        main(int(sys.argv[sys.argv.index("--calls") + 1]), write=False)
    else:
        main()
