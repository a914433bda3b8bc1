"""The C++ shim's RGB-D front end (shim/include/Objects.h, opencv_min.hpp; tests/cpp/test_rgbd.cpp):
Frame's RGB-D constructor -- the reference's signature and the raw-depth overload -- its monocular
constructor, Frame::ComputeStereoFromRGBD and cv::cvtColor, against the Python mirror and the literal
restatement (tests/rgbd_literal.py).

CPU: the driver builds, cv::Mat holds CV_16U / CV_8UC3 / CV_8UC4, the shim exports the reference's
members with the reference's signatures, and the GPU members fail loudly without a device.
"""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before liborbx.so is loaded: the library then binds to torch's HIP runtime)

import rgbd_literal as lit
from rgbd_literal import BF, DIST_TUM1, DIST_ZERO, K_TUM1, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "shim", "build", "test_rgbd")
CV_16U, CV_32F = 2, 5


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "shim")])
    return EXE


def test_rgbd_shim_abi(exe):
    r = subprocess.run([exe, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "abi ok" in r.stdout


def test_rgbd_shim_exports_reference_members(exe):
    out = subprocess.check_output(["nm", "-DC", "--defined-only", os.path.join(ROOT, "shim", "liborbx_shim.so")]).decode()
    for sym in [
            # include/Frame.h:58 (RGB-D) and :61 (monocular)
            "ORB_SLAM2::Frame::Frame(cv::Mat const&, cv::Mat const&, double const&, ORB_SLAM2::ORBextractor*, "
            "ORB_SLAM2::ORBVocabulary*, cv::Mat&, cv::Mat&, float const&, float const&)",
            "ORB_SLAM2::Frame::Frame(cv::Mat const&, double const&, ORB_SLAM2::ORBextractor*, "
            "ORB_SLAM2::ORBVocabulary*, cv::Mat&, cv::Mat&, float const&, float const&)",
            "ORB_SLAM2::Frame::ComputeStereoFromRGBD(cv::Mat const&)",
            "cv::cvtColor(cv::_InputArray const&, cv::_OutputArray const&, int, int)"]:
        assert sym in out, sym


def _payload(image, depth, factor, dist, rgb, ref_ctor):
    h, w = image.shape[:2]
    ch = 1 if image.ndim == 2 else image.shape[2]
    dtype = CV_16U if depth.dtype == np.uint16 else CV_32F
    return b"".join([struct.pack("<iiiiiiiff", w, h, lit.NFEATURES, ch, int(rgb), dtype, int(ref_ctor), float(factor), BF),
                     np.asarray(K_TUM1, f32).tobytes(), np.asarray(dist, f32).tobytes(),
                     np.ascontiguousarray(image).tobytes(), np.ascontiguousarray(depth).tobytes()])


def test_payload_layout():
    """The serialised scene has the size its parts add up to (no GPU)."""
    img = np.zeros((4, 6, 3), np.uint8)
    assert len(_payload(img, np.zeros((4, 6), np.uint16), 1.0, DIST_ZERO, True, False)) == 36 + 36 + 20 + 72 + 48
    assert len(_payload(img[..., 0], np.zeros((4, 6), f32), 1.0, DIST_ZERO, True, True)) == 36 + 36 + 20 + 24 + 96


class _Out:
    def __init__(self, data):
        self.d, self.o = data, 0

    def arr(self, dtype, n):
        a = np.frombuffer(self.d, dtype, n, self.o)
        self.o += a.nbytes
        return a

    def frame(self):
        from orb_slam2_commit_amd import KEYPOINT_DTYPE
        n = int(self.arr(np.int32, 1)[0])
        f = dict(keys=self.arr(KEYPOINT_DTYPE, n), desc=self.arr(np.uint8, n * 32).reshape(n, 32),
                 keys_un=self.arr(KEYPOINT_DTYPE, n), u_right=self.arr(f32, n), depth=self.arr(f32, n),
                 mb=self.arr(f32, 1)[0], log_sf=self.arr(f32, 1)[0], levels=int(self.arr(np.int32, 1)[0]))
        f["scale"] = self.arr(f32, f["levels"])
        f["inv_sigma2"] = self.arr(f32, f["levels"])
        return f


CASES = {
    # name: (channels, rgb, depth kind, distortion, the reference's constructor?)
    "colour_u16_tum1": (3, False, "u16", DIST_TUM1, False),
    "grey_f32_reference_ctor": (1, True, "f32", DIST_TUM1, True),
    "rgba_f32_half_nodist": (4, True, "f32_half", DIST_ZERO, False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_gpu_rgbd_frame_shim(gpu, exe, tmp_path, case):
    from orb_slam2_commit_amd import ORBextractor, frame_rgbd
    from orb_slam2_commit_amd.orb import compute_image_bounds
    ch, rgb, kind, dist, ref_ctor = CASES[case]
    colour = lit.colour_image(3, channels=max(ch, 3))
    grey = lit.gray(colour, rgb)
    image = grey if ch == 1 else colour
    depth, factor = lit.depth_scene(grey, kind)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(_payload(image, depth, factor, dist, rgb, ref_ctor))
    r = subprocess.run([exe, "rgbd", fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = _Out(open(fout, "rb").read())
    F = out.frame()
    statics = out.arr(f32, 12)
    M = out.frame()
    assert out.o == len(out.d)
    # the Python mirror and the literal
    ex = ORBextractor(lit.NFEATURES, 1.2, 8, 20, 7)
    mk, md, mun, mur, mz = frame_rgbd(ex, image, depth, factor, K_TUM1, dist, BF, rgb=rgb)
    wk, wd, wun, wur, wz = lit.reference(grey, depth, factor, K_TUM1, dist)
    assert len(F["keys"]) == len(mk) == len(wk) > 100
    for got, mirror, want, name in ((F["keys"], mk, wk, "mvKeys"), (F["desc"], md, wd, "mDescriptors"),
                                    (F["keys_un"], mun, wun, "mvKeysUn"), (F["u_right"], mur, wur, "mvuRight"),
                                    (F["depth"], mz, wz, "mvDepth")):
        assert np.array_equal(got.view(np.uint8), mirror.view(np.uint8)), name + " differs from the mirror's"
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), name + " differs from the literal's"
    # the monocular Frame: the same keypoints, no stereo information (the driver checked every -1)
    assert np.array_equal(M["keys"].view(np.uint8), wk.view(np.uint8)) and np.array_equal(M["desc"], wd)
    assert np.array_equal(M["keys_un"].view(np.uint8), wun.view(np.uint8))
    assert np.all(M["u_right"] == -1) and np.all(M["depth"] == -1)
    # scale tables, mb, and the first frame's statics
    fx, fy, cx, cy = K_TUM1[0, 0], K_TUM1[1, 1], K_TUM1[0, 2], K_TUM1[1, 2]
    for fr in (F, M):
        assert fr["levels"] == 8 and fr["mb"] == f32(BF) / fx
        assert abs(float(fr["log_sf"]) - float(np.log(np.float64(f32(1.2))))) <= 2.0 ** -24  # logf: half an ulp at 0.18
        assert np.array_equal(fr["scale"], ex.GetScaleFactors())
        assert np.array_equal(fr["inv_sigma2"], ex.GetInverseScaleSigmaSquares())
    b = [f32(v) for v in compute_image_bounds(lit.W, lit.H, K_TUM1, dist)]
    want_statics = [b[0], b[1], b[2], b[3], f32(64) / (b[1] - b[0]), f32(48) / (b[3] - b[2]), fx, fy, cx, cy,
                    f32(1) / fx, f32(1) / fy]
    assert np.array_equal(statics.view(np.uint32), np.asarray(want_statics, f32).view(np.uint32))
    ex.close()


@pytest.mark.gpu
def test_gpu_cvtcolor_shim(gpu, exe, tmp_path):
    w, h = 67, 9
    px4 = lit.colour_image(5, w, h, 4)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<ii", w, h) + px4.tobytes())
    r = subprocess.run([exe, "cvt", fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(fout, np.uint8).reshape(5, h, w)
    px3 = px4[..., :3]
    want = [lit.gray(px3, True), lit.gray(px3, False), lit.gray(px4, True), lit.gray(px4, False), lit.gray(px3, True)]
    for k, name in enumerate(["CV_RGB2GRAY", "CV_BGR2GRAY", "CV_RGBA2GRAY", "CV_BGRA2GRAY", "in place"]):
        assert np.array_equal(got[k], want[k]), name
