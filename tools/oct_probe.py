"""Per-phase cycles of the k_octree blocks on the bench batch (probe build:
tools/build_variant.sh oprobe -DORBX_OCT_PROBE; run with ORBX_LIB_OVERRIDE=build_ab/oprobe/liborbx.so).
Per level: the candidate pass before the rounds (pyramid path: histogram and the sums above it; generic
path: the load into LDS), the roots, the rounds by phase, the final pass (best response and output), the
blocks per path and the ticks blocks spent on the pyramid path before they left it."""
import ctypes as C
import sys

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import torch  # noqa: E402

from orb_slam2_commit_amd import ORBextractor, _lib, synth  # noqa: E402

W, H, B = 1241, 376, 256
WORDS = 12  # kOctProbeWords
dev = torch.device("cuda", 0)
pairs = [synth.stereo_pair(s, W, H) for s in synth.sequence_seeds(0, 16)]
images = torch.from_numpy(synth.stereo_batch(0, B, pairs=pairs)).to(dev)
ex = ORBextractor(2000, 1.2, 8, 20, 7)
cap = ex.max_keypoints(W, H)
kps = torch.empty((2 * B, cap, 28), dtype=torch.uint8, device=dev)
desc = torch.empty((2 * B, cap, 32), dtype=torch.uint8, device=dev)
counts = torch.zeros(2 * B, dtype=torch.int32, device=dev)
uR = torch.empty((B, cap), dtype=torch.float32, device=dev)
dep = torch.empty((B, cap), dtype=torch.float32, device=dev)
nm = torch.zeros(B, dtype=torch.int32, device=dev)
L = _lib.lib()
st = torch.cuda.current_stream()
ex.stereo_frames_device(images, kps, desc, counts, 386.1448, 386.1448 / 718.856, uR, dep, nm, st)
torch.cuda.synchronize()
buf = torch.zeros((2 * B * 8, WORDS), dtype=torch.int32, device=dev)
L.orbx_debug_oct_probe.argtypes = [C.c_void_p]
L.orbx_debug_oct_probe(C.c_void_p(buf.data_ptr()))
ex.stereo_frames_device(images, kps, desc, counts, 386.1448, 386.1448 / 718.856, uR, dep, nm, st)
torch.cuda.synchronize()
L.orbx_debug_oct_probe(None)
import numpy as np  # noqa: E402
a = buf.cpu().numpy().astype(np.int64).reshape(2 * B, 8, WORDS)
for l in range(8):
    x = a[:, l]
    print("level %d: T %6.0f  total %7.0f | first pass %6.0f roots %5.0f p1 %7.0f (%.1f rounds) p2 %7.0f (%.1f rounds) "
          "final %6.0f | blocks: pyramid %d generic %d empty %d, left the pyramid after %.0f ticks"
          % (l, x[:, 7].mean(), x[:, 6].mean(), x[:, 0].mean(), x[:, 1].mean(), x[:, 2].mean(), x[:, 3].mean(),
             x[:, 4].mean(), x[:, 5].mean(), x[:, 8].mean(), (x[:, 9] == 1).sum(), (x[:, 9] == 2).sum(),
             (x[:, 9] == 0).sum(), x[:, 10][x[:, 10] > 0].mean() if (x[:, 10] > 0).any() else 0))
tot = a[:, :, 6].sum()
print("share of block-ticks: first pass %.1f%% roots %.1f%% p1 %.1f%% p2 %.1f%% final %.1f%%; fallbacks %d of %d blocks" % (
    tuple(100.0 * a[:, :, i].sum() / tot for i in (0, 1, 2, 4, 8)) + (int(((a[:, :, 9] == 2) & (a[:, :, 10] > 0)).sum()), 2 * B * 8)))
