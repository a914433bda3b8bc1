"""KeyFrameDatabase relocalization-query latency on the GPU (recorded, not gated; bench.py is the gate).

Workload: 1,000 / 4,000 / 16,000 live keyframes of ~1,500 words each over a 2^20-word id space, laid
along a path (keyframe i takes its words from a window sliding over one long random word sequence, so
index neighbours share most of their words; the neighbour lists are the 10 nearest in index).  The
query frame is a keyframe in the middle of the map with 30% of its words replaced.  The BowVectors are
generated directly; the vocabulary is a flat one (2^20 leaves under the root) that only supplies the
word count.

Per size: orbx_kfdb_add throughput, the host form's median wall time per call (upload, 7 kernels,
read-back, one synchronisation), the device form's median time per call between HIP events on the
stream (queries queued back to back, nothing else on the device), the bytes a query has to read --
4 B per live pool entry for the vote plus 8 B per common word for the score -- the resulting GB/s and
that rate as a fraction of the device's stream-copy rate measured in the same run
(orbx_debug_hbm_copy).  Writes one JSON document (default profiles/kfdb_bench.json) and prints it.

Per-kernel times: the seven launches of a query are inside the library, so the script's own HIP events
bracket whole queries only.  The kernels' times come from a kernel trace of this script taken in a run
of its own (tracing slows the host, so the figures above are taken with the profiler off):

    rocprofv3 --kernel-trace --stats -d OUTDIR -o kfdb -- python tools/kfdb_bench.py --sizes 1000,16000 --out /dev/null
    python tools/kfdb_bench.py --aggregate-trace OUTDIR/kfdb_results.db --out profiles/kfdb_kernel_times.json

The second command needs no GPU: it reads the trace's SQLite database (view `kernels`: name, grid_x,
duration in ns), groups the k_kfdb_* launches by kernel and by map size (the two sizes differ in every
kernel's grid; for each kernel the smaller grid is the smaller map) and writes the median per launch.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_WORDS = 1 << 20
WORDS_PER_KF = 1500
STEP = 150


def flat_vocabulary_text(n_words):
    return "10 6 0 0\n" + ("0 1 " + "0 " * 32 + "1.0\n") * n_words


def make_map(rng, n_kf):
    seq = rng.integers(0, N_WORDS, n_kf * STEP + 2 * WORDS_PER_KF, dtype=np.int64)
    bows = []
    for i in range(n_kf):
        w = np.unique(seq[i * STEP:i * STEP + WORDS_PER_KF + 60])[:WORDS_PER_KF].astype(np.uint32)
        v = rng.random(len(w)) + 0.05
        bows.append((w, v / v.sum()))
    return bows


def make_query(rng, bow):
    w = bow[0]
    keep = w[rng.random(len(w)) < 0.7]
    w = np.unique(np.concatenate([keep, rng.integers(0, N_WORDS, len(bow[0]) - len(keep)).astype(np.uint32)]))
    v = rng.random(len(w)) + 0.05
    return w.astype(np.uint32), v / v.sum()


def aggregate_trace(db_path, out_path):
    """Median duration per launch of every query kernel in a rocprofv3 kernel trace of this script."""
    import sqlite3
    from collections import defaultdict
    con = sqlite3.connect(db_path)
    rows = con.execute("select name, grid_x, duration from kernels where name like '%k_kfdb_%' order by start").fetchall()
    by = defaultdict(lambda: defaultdict(list))
    for name, grid, ns in rows:
        short = name.split("(")[0].split("::")[-1]
        if short in ("k_kfdb_compact", "k_kfdb_bitmap", "k_kfdb_score"):
            continue  # not part of a candidate query
        by[short][int(grid)].append(ns)
    if not by:
        raise SystemExit("no k_kfdb_* launches in %s" % db_path)
    n_sizes = max(len(g) for g in by.values())
    out = dict(source="rocprofv3 --kernel-trace of tools/kfdb_bench.py, aggregated by its --aggregate-trace",
               unit="us, median per launch", maps=[])
    for rank in range(n_sizes):  # rank 0: the smallest map
        m = dict(launches_per_kernel=None, kernels={})
        for k in sorted(by):
            grids = sorted(by[k])
            # a kernel whose grid does not depend on the map size (k_kfdb_begin below 8,192 keyframes)
            # has one group for several maps: split it evenly in launch order
            if len(grids) == n_sizes:
                v = by[k][grids[rank]]
            else:
                allv = [x for g in grids for x in by[k][g]]
                per, rest = divmod(len(allv), n_sizes)
                if rest:
                    raise SystemExit("%s: %d launches do not split evenly over %d maps" % (k, len(allv), n_sizes))
                v = allv[rank * per:(rank + 1) * per]
            m["kernels"][k] = round(statistics.median(v) / 1e3, 2)
            # every query launches each of these kernels once: a kernel with another count was launched by
            # something else too, and the split above would have put its launches under the wrong map
            if m["launches_per_kernel"] not in (None, len(v)):
                raise SystemExit("map %d: %s has %d launches, the kernels before it %d: the trace is not of this "
                                 "script's run alone" % (rank, k, len(v), m["launches_per_kernel"]))
            m["launches_per_kernel"] = len(v)
        m["sum"] = round(sum(m["kernels"].values()), 2)
        out["maps"].append(m)
    text = json.dumps(out, indent=1)
    if out_path != "/dev/null":
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,4000,16000")
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfdb_bench.json"))
    ap.add_argument("--aggregate-trace", metavar="DB", help="aggregate a kernel trace of this script (no GPU needed)")
    a = ap.parse_args()
    if a.aggregate_trace:
        return aggregate_trace(a.aggregate_trace, a.out)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("kfdb_bench needs the GPU: no number is taken without one")
    from orb_slam2_commit_amd import KeyFrameDatabase, ORBVocabulary, _lib
    dev = torch.device("cuda:0")
    L = _lib.lib()

    # the device's own copy rate, same run
    n = 1 << 30
    src, dst, ms = torch.ones(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev), C.c_float()
    rates = []
    for _ in range(3):
        assert L.orbx_debug_hbm_copy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), n, 10, C.byref(ms)) == 0
        rates.append(2 * n / (ms.value / 1e3) / 1e9)
    copy_gbs = max(rates)
    del src, dst

    voc = ORBVocabulary()
    t0 = time.perf_counter()
    voc.loadFromText(flat_vocabulary_text(N_WORDS))
    load_s = time.perf_counter() - t0
    assert voc.n_words == N_WORDS
    out = dict(device=torch.cuda.get_device_name(0), n_words=N_WORDS, words_per_keyframe=WORDS_PER_KF,
               copy_rate_GBps=round(copy_gbs, 1), vocabulary_load_s=round(load_s, 2), calls=a.calls,
               warmup=a.warmup, sizes=[])
    rng = np.random.default_rng(1)
    for n_kf in [int(x) for x in a.sizes.split(",")]:
        bows = make_map(rng, n_kf)
        db = KeyFrameDatabase(voc)
        t0 = time.perf_counter()
        for i, b in enumerate(bows):
            db.add(i, b)
        add_s = time.perf_counter() - t0
        ids = list(range(n_kf))
        db.set_neighbours({i: [j for d in range(1, 6) for j in (i - d, i + d) if 0 <= j < n_kf][:10] for i in ids})
        q = make_query(rng, bows[n_kf // 2])
        all_words = np.concatenate([b[0] for b in bows])
        word_bytes = 4 * len(all_words)
        value_bytes = 8 * int(np.isin(all_words, q[0]).sum())
        fid = 1
        host_ms, cands = [], None
        for k in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            cands = db.DetectRelocalizationCandidates(fid, q)
            dt = (time.perf_counter() - t0) * 1e3
            fid += 1
            if k >= a.warmup:
                host_ms.append(dt)
        # device form: the query on the device, calls queued back to back on one stream
        dw = torch.from_numpy(q[0].view(np.int32)).to(dev)
        dv = torch.from_numpy(q[1]).to(dev)
        dn = torch.tensor([len(q[0])], dtype=torch.int32, device=dev)
        dc, dnc = torch.zeros(256, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        st = torch.cuda.Stream(dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.warmup + a.calls + 1)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(st):
            ev[0].record(st)
            for k in range(a.warmup + a.calls):
                db.reloc_candidates_device(fid, dw, dv, dn, dc, dnc, stream=st)
                fid += 1
                ev[k + 1].record(st)
        enqueue_ms = (time.perf_counter() - t0) * 1e3 / (a.warmup + a.calls)
        st.synchronize()
        dev_ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(a.warmup, a.warmup + a.calls)]
        got = [int(x) for x in dc[:int(dnc.item())].cpu().numpy()]
        assert got == cands, (got, cands)  # same query, same state-independent result
        med = statistics.median(dev_ms)
        gbs = (word_bytes + value_bytes) / (med / 1e3) / 1e9
        out["sizes"].append(dict(
            keyframes=n_kf, pool_entries=len(all_words), candidates=len(cands),
            add_per_s=round(n_kf / add_s), host_form_ms_median=round(statistics.median(host_ms), 4),
            host_form_ms_min=round(min(host_ms), 4), device_form_ms_median=round(med, 4),
            device_form_ms_min=round(min(dev_ms), 4), device_form_enqueue_ms=round(enqueue_ms, 4),
            word_bytes=word_bytes, value_bytes=value_bytes, scan_GBps=round(gbs, 1),
            fraction_of_copy_rate=round(gbs / copy_gbs, 4)))
        db.close()
    voc.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
