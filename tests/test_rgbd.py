"""The RGB-D front end: cvtColor to grey (k_cvt_gray), and Frame's RGB-D constructor -- extraction,
UndistortKeyPoints, convertTo at the lookup and ComputeStereoFromRGBD (k_rgbd_finish) -- against the
literal restatement in tests/rgbd_literal.py.

CPU tests pin the literal by hand-computed values and check that the scenes reach what they are
meant to reach; GPU tests hold orbx_cvt_gray, orbx_frame_rgbd and orbx_rgbd_frames_device to it bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import rgbd_literal as lit
from rgbd_literal import BF, DIST_TUM1, DIST_ZERO, FACTOR_5000, K_TUM1, f32

DISTS = {"nodist": DIST_ZERO, "tum1": DIST_TUM1}
DEPTH_KINDS = ("u16", "f32", "f32_half")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def scene():
    """The 320 x 240 colour scene, its grey image and its three depth scenes (built once, read only)."""
    colour = lit.colour_image(3)
    grey = lit.gray(colour, True)
    depth = {k: lit.depth_scene(grey, k) for k in DEPTH_KINDS}
    for a in (colour, grey, *[d for d, _ in depth.values()]):
        a.setflags(write=False)
    return dict(colour=colour, grey=grey, depth=depth)


# ------------------------------------------------------------------ CPU: the literal, by hand
def test_gray_kat():
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]], np.uint8)
    assert lit.gray(px, True).tolist() == [76, 150, 29, 255]
    assert lit.gray(px, False).tolist() == [29, 150, 76, 255]
    # alpha is ignored, whatever it holds
    px4 = np.concatenate([px, np.array([[0], [255], [7], [128]], np.uint8)], axis=1)
    assert lit.gray(px4, True).tolist() == [76, 150, 29, 255]
    assert lit.gray(px4, False).tolist() == [29, 150, 76, 255]
    # the rounding constant: (1*4899 + 8192) >> 14 = 0, and the first R that reaches 1 is ceil(8192/4899) = 2
    assert lit.gray(np.array([[1, 0, 0], [2, 0, 0]], np.uint8), True).tolist() == [0, 1]


def test_depth_rule_kat():
    fac = np.float32(1) / np.float32(5000)
    d = lit.convert_depth(np.uint16(5000), fac)
    assert d.dtype == np.float32 and d == np.float32(5000) * fac
    assert bits(d) == bits(np.float32(np.float32(5000.0) * fac))
    # a 16-bit image is converted even with factor 1 (its type is not CV_32F)
    assert lit.convert_depth(np.uint16(7), f32(1.0)) == f32(7.0)
    # f32 with factor 1: the bits pass through, a NaN payload included
    nan = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    assert bits(lit.convert_depth(nan, f32(1.0))) == 0x7FC12345
    assert bits(lit.convert_depth(f32(-0.0), f32(1.0))) == 0x80000000
    # the threshold is on |factor - 1| in float, compared in double
    assert not lit.factor_applies(f32(1.0)) and not lit.factor_applies(f32(1.0) + f32(5e-6))
    assert lit.factor_applies(f32(0.5)) and lit.factor_applies(FACTOR_5000) and lit.factor_applies(f32(1.00002))
    assert lit.convert_depth(f32(3.0), f32(0.5)) == f32(1.5)


def test_stereo_from_rgbd_kat():
    from orb_slam2_commit_amd import KEYPOINT_DTYPE
    keys = np.zeros(3, KEYPOINT_DTYPE)
    keys["x"], keys["y"] = [1.9, 0.2, 2.5], [0.9, 1.7, 1.5]  # truncation: pixels (0,1), (1,0), (1,2)
    un = keys.copy()
    un["x"] = [10.0, 20.0, 30.0]
    depth = np.array([[9, 2, 9], [4, 9, 0]], np.uint16)
    u_right, z = lit.stereo_from_rgbd(keys, un, depth, f32(0.5), 8.0)
    assert z.tolist() == [1.0, 2.0, -1.0]
    assert u_right.tolist() == [10.0 - 8.0 / 1.0, 20.0 - 8.0 / 2.0, -1.0]


def test_scene_conditions(scene):
    """What a scene must show before a pass on it means anything."""
    import oracle
    keys, _ = lit.oracle_keys(scene["grey"])
    assert len(keys) > 100
    x, y = keys["x"], keys["y"]
    assert np.any(x.astype(np.int64) != np.rint(x).astype(np.int64)), "truncation vs rounding never differs in x"
    assert np.any(y.astype(np.int64) != np.rint(y).astype(np.int64)), "truncation vs rounding never differs in y"
    un = oracle.undistort_keypoints(keys, K_TUM1, DIST_TUM1)
    moved = (un["x"].astype(np.int64) != x.astype(np.int64)) | (un["y"].astype(np.int64) != y.astype(np.int64))
    assert np.any(moved), "an index taken at the undistorted keypoint would read the same pixel"
    inside = (un["x"] >= 0) & (un["x"] < lit.W) & (un["y"] >= 0) & (un["y"] < lit.H) & moved
    d16, _ = scene["depth"]["u16"]
    assert np.any(d16[un["y"][inside].astype(np.int64), un["x"][inside].astype(np.int64)] !=
                  d16[y[inside].astype(np.int64), x[inside].astype(np.int64)]), "and would read the same depth"
    reached = set()
    for kind in DEPTH_KINDS:
        d, fac = scene["depth"][kind]
        reached |= lit.branches(keys, d, fac)
    assert reached == {"pos", "zero", "neg", "nan", "inf", "u16_max"}, reached
    assert lit.branches(keys, *scene["depth"]["u16"]) == {"pos", "zero", "u16_max"}
    assert lit.branches(keys, *scene["depth"]["f32"]) == {"pos", "zero", "neg", "nan", "inf"}
    # a swapped byte order and a leaking alpha channel would show
    assert np.any(lit.gray(scene["colour"], True) != lit.gray(scene["colour"], False))


# ------------------------------------------------------------------ GPU
def _padded(rng, shape, pitch, image_pitch):
    """uint8 buffer of len(shape[0]) images with the given row / image pitch, and the view of its pixels."""
    n, h, row = shape
    buf = rng.integers(0, 256, n * image_pitch + 8, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (n, h, row), (image_pitch, pitch, 1), writeable=True)
    return buf, view


@pytest.mark.gpu
@pytest.mark.parametrize("rgb", [True, False])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (67, 9), (333, 247)])
def test_gpu_cvt_gray(gpu, size, channels, rgb):
    """A batch of 3 images, source rows at a pitch that is no multiple of 4 and destination rows at a pitch
    above the width, from odd base addresses: byte-exact, the destination's padding untouched -- on the
    device entry point and on the host one."""
    import torch
    from orb_slam2_commit_amd import ORBextractor, _lib
    w, h = size
    n = 3
    rng = np.random.default_rng(w * 1000 + channels * 10 + rgb)
    sp = channels * w + 3 if (channels * w + 3) % 4 else channels * w + 5
    sip = sp * h + 1
    dp, dip = w + 7, (w + 7) * h + 5
    sbuf, src = _padded(rng, (n, h, channels * w), sp, sip)
    dbuf, _ = _padded(rng, (n, h, w), dp, dip)
    want = dbuf.copy()
    wv = np.lib.stride_tricks.as_strided(want[1:], (n, h, w), (dip, dp, 1))
    wv[...] = lit.gray(src.reshape(n, h, w, channels), rgb)
    L = _lib.lib()
    # device form, on the null stream, source and destination one byte off their allocations' alignment
    ex = ORBextractor(100, 1.2, 2, 20, 7)
    d_src = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), sbuf])).to(gpu)
    d_dst = torch.from_numpy(dbuf).to(gpu)
    _lib.check(L.orbx_cvt_gray_device(ex._h, C.c_void_p(d_src.data_ptr() + 1), sp, sip, n, w, h, channels, int(rgb),
                                      C.c_void_p(d_dst.data_ptr() + 1), dp, dip, C.c_void_p(1)), "orbx_cvt_gray_device")
    torch.cuda.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), want)
    # host form on the same layout
    got = dbuf.copy()
    _lib.check(L.orbx_cvt_gray(_lib.ptr(sbuf), sp, sip, n, w, h, channels, int(rgb), C.c_void_p(_lib.ptr(got).value + 1),
                               dp, dip, 0), "orbx_cvt_gray")
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_gpu_cvt_gray_mirror(gpu, scene):
    from orb_slam2_commit_amd import cvt_gray
    for ch in (3, 4):
        img = lit.colour_image(5, 67, 9, ch)
        for rgb in (True, False):
            assert np.array_equal(cvt_gray(img, rgb), lit.gray(img, rgb))
    batch = np.stack([scene["colour"], scene["colour"][::-1]])
    assert np.array_equal(cvt_gray(batch, False), lit.gray(batch, False))
    # a view with its own strides: every other column of rows twice as long
    wide = lit.colour_image(6, 40, 12, 3)
    assert np.array_equal(cvt_gray(wide[:, :20], True), lit.gray(wide[:, :20], True))


def _check_frame(got, want, what):
    keys, desc, un, u_right, z = got
    wk, wd, wun, wu, wz = want
    assert len(keys) == len(wk) > 100, (what, len(keys), len(wk))
    assert np.array_equal(keys.view(np.uint8), wk.view(np.uint8)), what + ": keypoints differ from the oracle's"
    assert np.array_equal(desc, wd), what + ": descriptors differ from the oracle's"
    assert np.array_equal(un.view(np.uint8), wun.view(np.uint8)), what + ": keys_un"
    assert np.array_equal(bits(z), bits(wz)), what + ": depth"
    assert np.array_equal(bits(u_right), bits(wu)), what + ": uRight"


@pytest.fixture(scope="module")
def extractor(gpu):
    from orb_slam2_commit_amd import ORBextractor
    ex = ORBextractor(lit.NFEATURES, 1.2, 8, 20, 7)
    yield ex
    ex.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dist", ["nodist", "tum1"])
@pytest.mark.parametrize("kind", DEPTH_KINDS)
def test_gpu_frame_rgbd(gpu, extractor, scene, kind, dist):
    from orb_slam2_commit_amd import frame_rgbd
    depth, fac = scene["depth"][kind]
    want = lit.reference(scene["grey"], depth, fac, K_TUM1, DISTS[dist])
    got = frame_rgbd(extractor, scene["grey"], depth, fac, K_TUM1, DISTS[dist], BF)
    _check_frame(got, want, kind + "/" + dist)
    # both outcomes occur: u16 has one patched keypoint without depth (raw 0; 65535 is a depth), f32 four
    assert (want[4] > 0).sum() > 100 and (want[4] == -1).sum() == (1 if kind == "u16" else 4)
    if kind == "f32":  # +inf passes d > 0 and gives uRight = kpU.x
        i = np.flatnonzero(np.isinf(got[4]))
        assert len(i) == 1 and got[3][i[0]] == got[2]["x"][i[0]]
    # level 0 of the handle's pyramid is the grey image
    assert np.array_equal(extractor.pyramid_level(0), scene["grey"])


@pytest.mark.gpu
@pytest.mark.parametrize("rgb", [True, False])
@pytest.mark.parametrize("channels", [3, 4])
def test_gpu_frame_rgbd_colour(gpu, extractor, scene, channels, rgb):
    """A colour input gives what its grey conversion gives when fed as one channel."""
    from orb_slam2_commit_amd import frame_rgbd
    depth, fac = scene["depth"]["u16"]
    colour = scene["colour"] if channels == 3 else lit.colour_image(3, channels=4)
    grey = lit.gray(colour, rgb)
    got = frame_rgbd(extractor, colour, depth, fac, K_TUM1, DIST_TUM1, BF, rgb=rgb)
    assert np.array_equal(extractor.pyramid_level(0), grey)
    one = frame_rgbd(extractor, grey, depth, fac, K_TUM1, DIST_TUM1, BF)
    for a, b in zip(got, one):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    if rgb:  # the module's scene: its depth scene was patched under these keypoints
        _check_frame(got, lit.reference(grey, depth, fac, K_TUM1, DIST_TUM1), "colour")


@pytest.mark.gpu
@pytest.mark.parametrize("null_stream", [False, True])
def test_gpu_rgbd_frames_device(gpu, extractor, scene, null_stream):
    """Three different frames (colour, 3 channels, a row pitch above the row) with different keypoint
    counts: per frame bit-equal to orbx_frame_rgbd and to the literal; slots beyond a frame's count are left
    as they were, as orbx_stereo_frames_device leaves them."""
    import torch
    from orb_slam2_commit_amd import KEYPOINT_DTYPE, frame_rgbd, rgbd_frames_device
    n, w, h = 3, lit.W, lit.H
    colours = [scene["colour"], lit.colour_image(8), (lit.colour_image(9) // 3 + 80).astype(np.uint8)]
    greys = [lit.gray(c, False) for c in colours]
    depths = [lit.depth_scene(g, "u16")[0] for g in greys]
    cap = extractor.max_keypoints(w, h)
    pad = torch.full((n, h + 1, w + 3, 3), 77, dtype=torch.uint8, device=gpu)
    pad[:, :h, :w] = torch.from_numpy(np.stack(colours)).to(gpu)
    dpad = torch.zeros((n, h, w + 2), dtype=torch.int16, device=gpu)
    dpad[:, :, :w] = torch.from_numpy(np.stack(depths).view(np.int16)).to(gpu)
    kps = torch.full((n, cap, 28), 0xAB, dtype=torch.uint8, device=gpu)
    kun = torch.full((n, cap, 28), 0xAB, dtype=torch.uint8, device=gpu)
    desc = torch.full((n, cap, 32), 0xAB, dtype=torch.uint8, device=gpu)
    cnt = torch.zeros(n, dtype=torch.int32, device=gpu)
    nm = torch.full((n,), -7, dtype=torch.int32, device=gpu)
    u_right = torch.full((n, cap), 123.0, dtype=torch.float32, device=gpu)
    z = torch.full((n, cap), 456.0, dtype=torch.float32, device=gpu)
    st = torch.cuda.current_stream() if null_stream else torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    rgbd_frames_device(extractor, pad[:, :h, :w], dpad[:, :, :w], FACTOR_5000, K_TUM1, DIST_TUM1, BF, kps, desc, cnt,
                       kun, u_right, z, nm, rgb=False, stream=st)
    torch.cuda.synchronize()
    counts = cnt.cpu().numpy()
    assert len(set(counts.tolist())) == n, counts
    for f in range(n):
        c = int(counts[f])
        got = (kps[f, :c].cpu().numpy().copy().view(KEYPOINT_DTYPE).ravel(), desc[f, :c].cpu().numpy(),
               kun[f, :c].cpu().numpy().copy().view(KEYPOINT_DTYPE).ravel(), u_right[f, :c].cpu().numpy(),
               z[f, :c].cpu().numpy())
        want = lit.reference(greys[f], depths[f], FACTOR_5000, K_TUM1, DIST_TUM1)
        _check_frame(got, want, "frame %d" % f)
        assert int(nm[f]) == int((want[4] > 0).sum())
        assert np.array_equal(extractor.pyramid_level(0, image=f), greys[f])
        assert bool((kun[f, c:] == 0xAB).all()) and bool((u_right[f, c:] == 123.0).all()) and bool((z[f, c:] == 456.0).all())
    for f in range(n):  # (after the batch's pyramid has been read: these calls replace it)
        one = frame_rgbd(extractor, colours[f], depths[f], FACTOR_5000, K_TUM1, DIST_TUM1, BF, rgb=False)
        _check_frame(one, lit.reference(greys[f], depths[f], FACTOR_5000, K_TUM1, DIST_TUM1), "one call, frame %d" % f)


@pytest.mark.gpu
def test_gpu_rgbd_error_paths(gpu, extractor, scene):
    from orb_slam2_commit_amd import _lib, frame_rgbd
    from orb_slam2_commit_amd.orb import camera
    L = _lib.lib()
    grey, (depth, fac) = scene["grey"], scene["depth"]["u16"]
    h, w = grey.shape
    cap = extractor.max_keypoints(w, h)
    from orb_slam2_commit_amd import KEYPOINT_DTYPE
    kps, kun = np.zeros(cap, KEYPOINT_DTYPE), np.zeros(cap, KEYPOINT_DTYPE)
    desc, u_right, z = np.zeros((cap, 32), np.uint8), np.zeros(cap, f32), np.zeros(cap, f32)
    cam = camera(K_TUM1, DIST_TUM1)
    n = C.c_int(-1)

    def call(img, dw, dh, dtype, channels=1):
        return L.orbx_frame_rgbd(extractor._h, _lib.ptr(img) if img is not None else None, w * channels, w, h, channels,
                                 1, _lib.ptr(depth), 2 * w, dw, dh, dtype, C.c_float(fac), C.byref(cam), C.c_float(BF),
                                 _lib.ptr(kps), _lib.ptr(desc), cap, C.byref(n), _lib.ptr(kun), _lib.ptr(u_right),
                                 _lib.ptr(z))
    assert call(grey, w - 1, h, _lib.ORBX_DEPTH_U16) == _lib.ORBX_ERR_ARG
    assert call(grey, w, h + 1, _lib.ORBX_DEPTH_U16) == _lib.ORBX_ERR_ARG
    assert call(grey, w, h, 0) == _lib.ORBX_ERR_ARG  # CV_8U
    assert call(grey, w, h, 6) == _lib.ORBX_ERR_ARG  # CV_64F
    assert call(grey, w, h, _lib.ORBX_DEPTH_U16, channels=2) == _lib.ORBX_ERR_ARG
    assert call(None, w, h, _lib.ORBX_DEPTH_U16) == _lib.ORBX_OK and n.value == 0  # an empty image
    # the mirror on an empty image
    e = frame_rgbd(extractor, np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.uint16), fac, K_TUM1, DIST_TUM1, BF)
    assert len(e[0]) == 0 and e[1] is None and len(e[3]) == 0
    # cvtColor is not called on one channel
    out = np.zeros((h, w), np.uint8)
    assert L.orbx_cvt_gray(_lib.ptr(grey), w, w * h, 1, w, h, 1, 1, _lib.ptr(out), w, w * h, 0) == _lib.ORBX_ERR_ARG
    assert L.orbx_cvt_gray_device(extractor._h, _lib.ptr(grey), w, w * h, 1, w, h, 1, 1, _lib.ptr(out), w, w * h,
                                  None) == _lib.ORBX_ERR_ARG
    colour = scene["colour"]
    assert L.orbx_cvt_gray(_lib.ptr(colour), 3 * w - 1, 3 * w * h, 1, w, h, 3, 1, _lib.ptr(out), w, w * h,
                           0) == _lib.ORBX_ERR_ARG  # a pitch below the row
    # a good call still works on the handle afterwards
    assert call(grey, w, h, _lib.ORBX_DEPTH_U16) == _lib.ORBX_OK and n.value > 100
