"""Per-phase s_memtime ticks of the resize blocks on the bench batch, per kernel and level (probe build:
tools/build_variant.sh rzprobe -DORBX_RZ_PROBE; run with ORBX_LIB_OVERRIDE=build_ab/rzprobe/liborbx.so).
A probe build of an older tree gives that tree's split with the same tool."""
import ctypes as C
import sys

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from orb_slam2_commit_amd import ORBextractor, _lib, synth  # noqa: E402

W, H, B = 1241, 376, 64
dev = torch.device("cuda", 0)
pairs = [synth.stereo_pair(s, W, H) for s in synth.sequence_seeds(0, 16)]
images = torch.from_numpy(synth.stereo_batch(0, B, pairs=pairs)).to(dev)
ex = ORBextractor(2000, 1.2, 8, 20, 7)
cap = ex.max_keypoints(W, H)
kps = torch.empty((2 * B, cap, 28), dtype=torch.uint8, device=dev)
desc = torch.empty((2 * B, cap, 32), dtype=torch.uint8, device=dev)
counts = torch.zeros(2 * B, dtype=torch.int32, device=dev)
st = torch.cuda.current_stream()
ex.extract_batch_device(images, kps, desc, counts, st)  # warm-up
torch.cuda.synchronize()
# at most (w / 128 + 1) * (h / 32 + 1) blocks per level and image, whichever kernel runs it
nblocks = 2 * B * sum((int(W / 1.2 ** l) // 128 + 2) * (int(H / 1.2 ** l) // 32 + 2) for l in range(1, 8))
buf = torch.zeros((nblocks, 8), dtype=torch.int32, device=dev)
L = _lib.lib()
L.orbx_debug_rz_probe.argtypes = [C.c_void_p, C.c_uint]
assert L.orbx_debug_rz_probe(C.c_void_p(buf.data_ptr()), nblocks) == 0
ex.extract_batch_device(images, kps, desc, counts, st)
torch.cuda.synchronize()
L.orbx_debug_rz_probe(None, 0)
a = buf.cpu().numpy().astype(np.int64)
a = a[a[:, 6] == 1]
names = ["footprint -> LDS", "horizontal pass", "arithmetic + stores issued", "store drain"]
print("%d blocks (s_memtime ticks, first wave of each block)" % len(a))
for path, kname in ((0, "k_resize"), (1, "k_resize_strip")):
    k = a[a[:, 5] == path]
    if not len(k):
        continue
    tot = k[:, :4].sum(1)
    print("%s: %d blocks, ticks per block mean %.1f median %.0f" % (kname, len(k), tot.mean(), np.median(tot)))
    for i, n in enumerate(names):
        print("  %-28s mean %7.1f median %5.0f  %5.1f %%" % (n, k[:, i].mean(), np.median(k[:, i]), 100.0 * k[:, i].sum() / tot.sum()))
    for l in sorted(set(k[:, 4])):
        kl = k[k[:, 4] == l]
        print("  level %d: %6d blocks, mean ticks %s" % (l, len(kl), " ".join("%6.1f" % v for v in kl[:, :4].mean(0))))
