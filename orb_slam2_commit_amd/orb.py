"""Host-side mirror of the reference's hot-path classes over liborbx.so.

Names, argument meaning and error behaviour follow the reference:

* ``ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)``
  (include/ORBextractor.h:77) with ``__call__(image, mask)`` ==
  ``operator()`` (src/ORBextractor.cc:1138-1211), ``GetLevels``,
  ``GetScaleFactor(s)``, ``GetInverseScaleFactors``, ``GetScaleSigmaSquares``,
  ``GetInverseScaleSigmaSquares`` and ``mvImagePyramid``.
* ``ORBmatcher.DescriptorDistance`` (src/ORBmatcher.cc:1844-1860), batched.
* ``compute_stereo_matches`` == ``Frame::ComputeStereoMatches``
  (src/Frame.cc:547-788).
* ``ORBmatcher.SearchByBoW`` (src/ORBmatcher.cc:175-325, 589-736).
* ``Optimizer.LocalBundleAdjustment`` (src/Optimizer.cc:530-885) on an
  explicit problem (cameras, points, observations) gathered like the
  reference gathers it from the covisibility graph.

Every result is computed by the HIP kernels; this module only moves bytes.
"""
import contextlib
import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import KEYPOINT_DTYPE, check, ptr

TH_HIGH = 100  # src/ORBmatcher.cc:37
TH_LOW = 50    # src/ORBmatcher.cc:38
HISTO_LENGTH = 30  # src/ORBmatcher.cc:39


class ORBextractor:
    """GPU ORB extractor with the reference constructor signature."""

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device=0):
        L = _lib.lib()
        self.params = _lib.ExtractorParams(int(nfeatures), float(scaleFactor), int(nlevels), int(iniThFAST),
                                           int(minThFAST))
        h = C.c_void_p()
        check(L.orbx_extractor_create(C.byref(self.params), int(device), C.byref(h)), "orbx_extractor_create")
        self._h = h
        self.nfeatures = int(nfeatures)
        self.scaleFactor = float(scaleFactor)
        self.nlevels = int(nlevels)
        self.device = int(device)
        n = self.nlevels
        self._tables = [np.zeros(n, np.float32) for _ in range(4)]
        check(L.orbx_extractor_scale_tables(h, *[ptr(t) for t in self._tables]), "orbx_extractor_scale_tables")
        self._last_shape = None

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().orbx_extractor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- reference accessors (include/ORBextractor.h:82-104)
    def GetLevels(self):
        return _lib.lib().orbx_extractor_get_levels(self._h)

    def GetScaleFactor(self):
        return self.scaleFactor

    def GetScaleFactors(self):
        return self._tables[0].copy()

    def GetInverseScaleFactors(self):
        return self._tables[1].copy()

    def GetScaleSigmaSquares(self):
        return self._tables[2].copy()

    def GetInverseScaleSigmaSquares(self):
        return self._tables[3].copy()

    def max_keypoints(self, width, height):
        n = _lib.lib().orbx_extractor_max_keypoints(self._h, int(width), int(height))
        if n < 0:
            check(n, "orbx_extractor_max_keypoints")
        return n

    # --- ORBextractor::operator()
    def __call__(self, image, mask=None):
        """Returns (keypoints structured array [cv::KeyPoint layout], descriptors uint8[n,32] or None).

        ``mask`` is accepted and ignored, as in the reference."""
        if image is None or getattr(image, "size", 0) == 0:
            return np.zeros(0, KEYPOINT_DTYPE), None
        img = np.asarray(image)
        assert img.dtype == np.uint8 and img.ndim == 2, "image must be CV_8UC1"  # src/ORBextractor.cc:1146
        h, w = img.shape
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        cap = self.max_keypoints(w, h)
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        check(_lib.lib().orbx_extract(self._h, ptr(img), w, h, img.strides[0], ptr(kps), cap, ptr(desc), C.byref(n)),
              "orbx_extract")
        self._last_shape = (w, h)
        n = n.value
        if n == 0:
            return kps[:0].copy(), None  # descriptors.release(), src/ORBextractor.cc:1163-1164
        return kps[:n].copy(), desc[:n].copy()

    @property
    def mvImagePyramid(self):
        return [self.pyramid_level(l) for l in range(self.nlevels)]

    def pyramid_level(self, level, image=0):
        L = _lib.lib()
        w, h = C.c_int(0), C.c_int(0)
        check(L.orbx_pyramid_level(self._h, image, level, None, 0, C.byref(w), C.byref(h)), "orbx_pyramid_level")
        out = np.zeros((h.value, w.value), np.uint8)
        check(L.orbx_pyramid_level(self._h, image, level, ptr(out), w.value, C.byref(w), C.byref(h)),
              "orbx_pyramid_level")
        return out

    # --- device batch API (inputs/outputs are torch CUDA tensors)
    def extract_batch_device(self, images, kps, desc, counts, stream=None):
        """images: uint8 [n,H,W] device tensor; kps: uint8 [n,cap,28]; desc: uint8 [n,cap,32]; counts: int32 [n]."""
        n, h, w = images.shape
        cap = kps.shape[1]
        check(_lib.lib().orbx_extract_batch_device(self._h, n, ptr(images), w, h, h * w, ptr(kps), ptr(desc),
                                                   ptr(counts), cap, _stream_ptr(stream, True)),
              "orbx_extract_batch_device")

    def stereo_frames_device(self, images, kps, desc, counts, bf, baseline, uright, depth, nmatches, stream=None):
        """images: uint8 [2n,H,W] ordered L0,R0,L1,R1...; uright/depth: float32 [n,cap]; nmatches: int32 [n]."""
        n2, h, w = images.shape
        cap = kps.shape[1]
        check(_lib.lib().orbx_stereo_frames_device(self._h, n2 // 2, ptr(images), w, h, h * w, ptr(kps), ptr(desc),
                                                   ptr(counts), cap, C.c_float(bf), C.c_float(baseline),
                                                   ptr(uright), ptr(depth), ptr(nmatches), _stream_ptr(stream, True)),
              "orbx_stereo_frames_device")


def _stream_ptr(stream, handle_api=False):
    """hipStream_t of a torch stream.  For the handle-owning entry points (extractor, vocabulary) NULL
    would pick the handle's own non-blocking stream, so torch's legacy default stream (cuda_stream 0) is
    passed as ORBX_STREAM_NULL to keep the caller's work on that stream ordered with the library's."""
    if stream is None:
        return None
    s = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
    if s == 0 and handle_api:
        return C.c_void_p(1)  # ORBX_STREAM_NULL
    return C.c_void_p(s)


def compute_stereo_matches(extractor_left, extractor_right, kps_left, desc_left, kps_right, desc_right, bf,
                           baseline):
    """Frame::ComputeStereoMatches on the pyramids of the extractors' last calls.

    Returns (mvuRight float32[N], mvDepth float32[N]) with -1 for no match."""
    nL, nR = len(kps_left), len(kps_right)
    uR = np.full(nL, -1.0, np.float32)
    depth = np.full(nL, -1.0, np.float32)
    if nL == 0:
        return uR, depth
    kL = np.ascontiguousarray(kps_left, KEYPOINT_DTYPE)
    kR = np.ascontiguousarray(kps_right, KEYPOINT_DTYPE)
    dL = np.ascontiguousarray(desc_left, np.uint8)
    dR = np.ascontiguousarray(desc_right if desc_right is not None else np.zeros((0, 32), np.uint8), np.uint8)
    check(_lib.lib().orbx_stereo_match(extractor_left._h, extractor_right._h, ptr(kL), ptr(dL), nL, ptr(kR),
                                       ptr(dR), nR, C.c_float(bf), C.c_float(baseline), ptr(uR), ptr(depth)),
          "orbx_stereo_match")
    return uR, depth


def debug_stereo_keypoints(extractor_left, extractor_right, kps_left, desc_left, kps_right, desc_right, bf,
                           baseline):
    """The shipped matcher on SUPPLIED keypoints and descriptors (orbx_debug_stereo_keypoints, tests
    only), over the pyramids of the extractors' last calls.

    Returns (mvuRight float32[N], mvDepth float32[N], sad int32[N] (-1 unless accepted before the median
    filter), matches kept)."""
    nL, nR = len(kps_left), len(kps_right)
    uR = np.full(nL, -1.0, np.float32)
    depth = np.full(nL, -1.0, np.float32)
    sad = np.full(nL, -1, np.int32)
    nm = np.zeros(1, np.int32)
    kL = np.ascontiguousarray(kps_left, KEYPOINT_DTYPE)
    kR = np.ascontiguousarray(kps_right, KEYPOINT_DTYPE)
    dL = np.ascontiguousarray(desc_left if desc_left is not None else np.zeros((0, 32), np.uint8), np.uint8)
    dR = np.ascontiguousarray(desc_right if desc_right is not None else np.zeros((0, 32), np.uint8), np.uint8)
    assert dL.shape == (nL, 32) and dR.shape == (nR, 32)
    check(_lib.lib().orbx_debug_stereo_keypoints(extractor_left._h, extractor_right._h, ptr(kL), ptr(dL), nL,
                                                 ptr(kR), ptr(dR), nR, C.c_float(bf), C.c_float(baseline), ptr(uR),
                                                 ptr(depth), ptr(sad), ptr(nm)),
          "orbx_debug_stereo_keypoints")
    return uR, depth, sad, int(nm[0])


def debug_launch_plan(params, width, height, what, a0=0, a1=0, a2=0):
    """Item `what` (ORBX_LP_*) of the plan of one image geometry, built on the host: int64 words."""
    L = _lib.lib()
    n = L.orbx_debug_launch_plan(C.byref(params), int(width), int(height), int(what), a0, a1, a2, None, 0)
    if n < 0:
        check(n, "orbx_debug_launch_plan")
    out = np.zeros(n, np.int64)
    L.orbx_debug_launch_plan(C.byref(params), int(width), int(height), int(what), a0, a1, a2, ptr(out), n)
    return out


def debug_octree_candidates(extractor, cell_counts, candidates):
    """The shipped k_octree on SUPPLIED FAST candidates (orbx_debug_octree_candidates, tests only), on
    the geometry of the extractor's last call.  cell_counts int32[n_img, ncells], candidates
    uint32[n_img, cand_total] in ORBX_DBG_CANDIDATES' logical view.

    Returns (oct_count int32[n_img, nlevels], oct_out uint32[n_img, oct_total])."""
    counts = np.ascontiguousarray(cell_counts, np.int32)
    cand = np.ascontiguousarray(candidates, np.uint32)
    w, h = extractor._last_shape
    cells = debug_launch_plan(extractor.params, w, h, 11).reshape(-1, 8)  # ORBX_LP_CELLS
    levels = debug_launch_plan(extractor.params, w, h, 12).reshape(-1, 8)  # ORBX_LP_OCT_LEVELS
    n_img = len(counts)
    assert counts.shape == (n_img, len(cells)) and cand.shape == (n_img, int(cells[:, 6].sum()))
    oct_count = np.zeros((n_img, extractor.nlevels), np.int32)
    oct_out = np.zeros((n_img, int(levels[:, 7].sum())), np.uint32)
    check(_lib.lib().orbx_debug_octree_candidates(extractor._h, n_img, ptr(counts), ptr(cand), ptr(oct_count),
                                                  ptr(oct_out)), "orbx_debug_octree_candidates")
    return oct_count, oct_out


def debug_octree_paths(extractor, cell_counts, candidates, depth_cap=-1):
    """debug_octree_candidates' launch through orbx_debug_octree_paths, which also reports the path each
    (image, level) block took: 0 an empty level, 1 the count pyramid, 2 the generic path.  depth_cap >= 0
    runs the launch groups at min(plan's D, depth_cap); 0 is the generic path alone.

    Returns (oct_count int32[n_img, nlevels], oct_out uint32[n_img, oct_total], paths int32[n_img, nlevels])."""
    counts = np.ascontiguousarray(cell_counts, np.int32)
    cand = np.ascontiguousarray(candidates, np.uint32)
    w, h = extractor._last_shape
    cells = debug_launch_plan(extractor.params, w, h, 11).reshape(-1, 8)  # ORBX_LP_CELLS
    levels = debug_launch_plan(extractor.params, w, h, 12).reshape(-1, 8)  # ORBX_LP_OCT_LEVELS
    n_img = len(counts)
    assert counts.shape == (n_img, len(cells)) and cand.shape == (n_img, int(cells[:, 6].sum()))
    oct_count = np.zeros((n_img, extractor.nlevels), np.int32)
    oct_out = np.zeros((n_img, int(levels[:, 7].sum())), np.uint32)
    paths = np.zeros((n_img, extractor.nlevels), np.int32)
    check(_lib.lib().orbx_debug_octree_paths(extractor._h, n_img, ptr(counts), ptr(cand), int(depth_cap),
                                             ptr(oct_count), ptr(oct_out), ptr(paths)), "orbx_debug_octree_paths")
    return oct_count, oct_out, paths


def frame_stereo(extractor, image_left, image_right, bf, baseline):
    """The ORB part of Frame's stereo constructor (src/Frame.cc:62-123: ExtractORB(0/1) + ComputeStereoMatches)
    in one call through `extractor` (both images as one batch of two, one copy back).

    Returns (kps_left, desc_left, kps_right, desc_right, mvuRight, mvDepth) as ``extractor(image)`` and
    ``compute_stereo_matches`` return them (descriptors None for an empty side)."""
    L = np.asarray(image_left)
    R = np.asarray(image_right)
    assert L.dtype == np.uint8 and L.ndim == 2 and R.dtype == np.uint8 and R.shape == L.shape, "two CV_8UC1 images"
    if L.strides[1] != 1:
        L = np.ascontiguousarray(L)
    if R.strides[1] != 1:
        R = np.ascontiguousarray(R)
    h, w = L.shape
    cap = extractor.max_keypoints(w, h)
    kL, kR = np.zeros(cap, KEYPOINT_DTYPE), np.zeros(cap, KEYPOINT_DTYPE)
    dL, dR = np.zeros((cap, 32), np.uint8), np.zeros((cap, 32), np.uint8)
    uR, depth = np.full(cap, -1.0, np.float32), np.full(cap, -1.0, np.float32)
    nL, nR = C.c_int(0), C.c_int(0)
    check(_lib.lib().orbx_frame_stereo(extractor._h, ptr(L), L.strides[0], ptr(R), R.strides[0], w, h, C.c_float(bf),
                                       C.c_float(baseline), ptr(kL), ptr(dL), cap, C.byref(nL), ptr(kR), ptr(dR), cap,
                                       C.byref(nR), ptr(uR), ptr(depth)),
          "orbx_frame_stereo")
    extractor._last_shape = (w, h)
    nL, nR = nL.value, nR.value
    return (kL[:nL].copy(), dL[:nL].copy() if nL else None, kR[:nR].copy(), dR[:nR].copy() if nR else None,
            uR[:nL].copy(), depth[:nL].copy())


def cvt_gray(image, rgb, device=0):
    """cv::cvtColor(image, gray, CV_RGB2GRAY / CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY), the first statements
    of Tracking::GrabImage* (src/Tracking.cc:174-199, 215-228, 246-259).  image: uint8 [H, W, 3 or 4] or a batch
    [n, H, W, 3 or 4] (row and image strides are the array's own; a pixel's bytes adjacent); rgb: mbRGB.
    Returns uint8 [H, W] or [n, H, W]."""
    a = np.asarray(image)
    assert a.dtype == np.uint8 and a.ndim in (3, 4), "image must be CV_8UC3 / CV_8UC4 (or a batch of them)"
    b = a if a.ndim == 4 else a[None]
    n, h, w, c = b.shape
    if b.size and (b.strides[3] != 1 or b.strides[2] != c or b.strides[1] < w * c or
                   (n > 1 and b.strides[0] < (h - 1) * b.strides[1] + w * c)):
        b = np.ascontiguousarray(b)
    out = np.zeros((n, h, w), np.uint8)
    check(_lib.lib().orbx_cvt_gray(ptr(b), b.strides[1], b.strides[0], n, w, h, c, int(bool(rgb)), ptr(out), w,
                                   w * h, int(device)), "orbx_cvt_gray")
    return out if a.ndim == 4 else out[0]


def _depth_type(depth):
    if depth.dtype == np.uint16:
        return _lib.ORBX_DEPTH_U16
    if depth.dtype == np.float32:
        return _lib.ORBX_DEPTH_F32
    raise TypeError("depth image must be CV_16U or CV_32F, not %s" % depth.dtype)


def frame_rgbd(extractor, image, depth, depth_factor, K, dist_coef, bf, rgb=True):
    """The ORB part of Frame's RGB-D constructor (src/Frame.cc:126-183: ExtractORB(0), UndistortKeyPoints,
    ComputeStereoFromRGBD) with Tracking::GrabImageRGBD's preprocessing (src/Tracking.cc:210-233: cvtColor,
    convertTo(CV_32F, mDepthMapFactor)) in one call through `extractor`.

    image: uint8 [H, W] or [H, W, 3 or 4] (rgb: mbRGB); depth: uint16 or float32 [H, W]; depth_factor:
    mDepthMapFactor as Tracking holds it (already inverted, src/Tracking.cc:144-148).
    Returns (kps, desc, kps_un, mvuRight, mvDepth); descriptors None without keypoints."""
    img = np.asarray(image)
    dep = np.asarray(depth)
    assert img.dtype == np.uint8 and img.ndim in (2, 3), "image must be CV_8UC1 / C3 / C4"
    ch = 1 if img.ndim == 2 else img.shape[2]
    if img.size and (img.strides[1] != ch or (img.ndim == 3 and img.strides[2] != 1)):
        img = np.ascontiguousarray(img)
    assert dep.ndim == 2
    if dep.size and dep.strides[1] != dep.itemsize:
        dep = np.ascontiguousarray(dep)
    h, w = img.shape[:2]
    cap = max(extractor.max_keypoints(w, h), 1) if w > 0 and h > 0 else 1
    kps, kun = np.zeros(cap, KEYPOINT_DTYPE), np.zeros(cap, KEYPOINT_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    uR, d = np.full(cap, -1.0, np.float32), np.full(cap, -1.0, np.float32)
    n = C.c_int(0)
    cam = camera(K, dist_coef)
    check(_lib.lib().orbx_frame_rgbd(extractor._h, ptr(img) if img.size else None, img.strides[0], w, h, ch,
                                     int(bool(rgb)), ptr(dep), dep.strides[0], dep.shape[1], dep.shape[0],
                                     _depth_type(dep), C.c_float(depth_factor), C.byref(cam), C.c_float(bf),
                                     ptr(kps), ptr(desc), cap, C.byref(n), ptr(kun), ptr(uR), ptr(d)),
          "orbx_frame_rgbd")
    extractor._last_shape = (w, h)
    n = n.value
    return kps[:n].copy(), desc[:n].copy() if n else None, kun[:n].copy(), uR[:n].copy(), d[:n].copy()


def rgbd_frames_device(extractor, images, depth, depth_factor, K, dist_coef, bf, kps, desc, counts, kps_un, uright,
                       depth_out, nmatches, rgb=True, stream=None):
    """orbx_rgbd_frames_device: n RGB-D frames resident on the device (torch tensors).

    images: uint8 [n, H, W] or [n, H, W, 3 or 4]; depth: int16 / uint16 bits or float32 [n, H, W] (a torch
    int16 tensor holds CV_16U bits); kps / kps_un: uint8 [n, cap, 28]; desc: uint8 [n, cap, 32]; counts /
    nmatches: int32 [n]; uright / depth_out: float32 [n, cap].  Row and image strides are the tensors' own."""
    n, h, w = images.shape[:3]
    ch = 1 if images.dim() == 3 else images.shape[3]
    assert images.stride(2) == ch and (ch == 1 or images.stride(3) == 1) and depth.stride(2) == 1
    es = depth.element_size()
    dtype = _lib.ORBX_DEPTH_U16 if es == 2 else _lib.ORBX_DEPTH_F32
    assert es == 2 or depth.is_floating_point(), "depth must be 16-bit integer or float32"
    cam = camera(K, dist_coef)
    check(_lib.lib().orbx_rgbd_frames_device(extractor._h, n, ptr(images), w, h, ch, int(bool(rgb)), images.stride(1),
                                             images.stride(0), ptr(depth), dtype, depth.stride(1) * es,
                                             depth.stride(0) * es, C.c_float(depth_factor), C.byref(cam),
                                             C.c_float(bf), ptr(kps), ptr(desc), ptr(counts), kps.shape[1],
                                             ptr(kps_un), ptr(uright), ptr(depth_out), ptr(nmatches),
                                             _stream_ptr(stream, True)),
          "orbx_rgbd_frames_device")


def compute_distinctive_descriptors(desc, obs_off, device=0):
    """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:249-320) for a batch of MapPoints:
    desc[obs_off[p]:obs_off[p+1]] are point p's observed descriptors in mObservations order.
    Returns (best[n_points] int32, -1 where a point has no observation; mDescriptor[n_points, 32])."""
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    off = np.ascontiguousarray(obs_off, np.int32)
    n = len(off) - 1
    best = np.zeros(max(n, 1), np.int32)
    out = np.zeros((max(n, 1), 32), np.uint8)
    check(_lib.lib().orbx_distinctive_descriptors(ptr(d), ptr(off), n, ptr(best), ptr(out), int(device)),
          "orbx_distinctive_descriptors")
    return best[:n], out[:n]


def camera(K, dist_coef):
    """orbx_camera from mK (3x3) and mDistCoef (4 or 5 coefficients)."""
    d = np.asarray(dist_coef, np.float32).reshape(-1)
    cam = _lib.Camera()
    cam.K[:] = _f32(K).reshape(9).tolist()
    dd = np.zeros(5, np.float32)
    dd[:len(d)] = d
    cam.dist[:] = dd.tolist()
    cam.n_dist = len(d)
    return cam


def undistort_keypoints(keys, K, dist_coef, device=0):
    """Frame::UndistortKeyPoints (src/Frame.cc:471-506): mvKeysUn from mvKeys, mK and mDistCoef."""
    k = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    out = np.zeros(max(len(k), 1), KEYPOINT_DTYPE)
    cam = camera(K, dist_coef)
    check(_lib.lib().orbx_undistort_keypoints(ptr(k), len(k), C.byref(cam), ptr(out), int(device)),
          "orbx_undistort_keypoints")
    return out[:len(k)]


def compute_image_bounds(cols, rows, K, dist_coef, device=0):
    """Frame::ComputeImageBounds (src/Frame.cc:508-537): (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    if float(np.float32(np.asarray(dist_coef, np.float32).reshape(-1)[0])) == 0.0:
        return 0.0, float(cols), 0.0, float(rows)
    c = np.zeros(4, KEYPOINT_DTYPE)
    c["x"] = [0.0, cols, 0.0, cols]
    c["y"] = [0.0, 0.0, rows, rows]
    u = undistort_keypoints(c, K, dist_coef, device)
    return (float(min(u["x"][0], u["x"][2])), float(max(u["x"][1], u["x"][3])),
            float(min(u["y"][0], u["y"][1])), float(max(u["y"][2], u["y"][3])))


def bow_side(side):
    """dict(desc, angle, valid, node_id, node_off, feat) -> (orbx_bow_side, keep-alive arrays)."""
    arrs = dict(desc=np.ascontiguousarray(side["desc"], np.uint8),
                angle=np.ascontiguousarray(side["angle"], np.float32),
                valid=None if side.get("valid") is None else np.ascontiguousarray(side["valid"], np.uint8),
                node_id=np.ascontiguousarray(side["node_id"], np.uint32),
                node_off=np.ascontiguousarray(side["node_off"], np.int32),
                feat=np.ascontiguousarray(side["feat"], np.int32))
    s = _lib.BowSide(len(arrs["desc"]), ptr(arrs["desc"]), ptr(arrs["angle"]), ptr(arrs["valid"]),
                     len(arrs["node_id"]), ptr(arrs["node_id"]), ptr(arrs["node_off"]), ptr(arrs["feat"]))
    return s, arrs


class ORBmatcher:
    """ORBmatcher(nnratio=0.6, checkOri=True) -- include/ORBmatcher.h:47."""

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        self.device = int(device)

    def SearchByBoW(self, side_a, side_b, kf_kf=False):
        """SearchByBoW(KeyFrame*, Frame&) (kf_kf=False) or SearchByBoW(KeyFrame*, KeyFrame*) (kf_kf=True).

        Sides are dicts (desc, angle, valid, node_id, node_off, feat).  Returns (match, nmatches):
        KF-F: match[i_frame] = KF feature index or -1; KF-KF: match[i_kf1] = KF2 feature index or -1."""
        A, ka = bow_side(side_a)
        B, kb = bow_side(side_b)
        nout = A.n if kf_kf else B.n
        match = np.zeros(nout, np.int32)
        n = C.c_int(0)
        fn = _lib.lib().orbx_search_by_bow_kf_kf if kf_kf else _lib.lib().orbx_search_by_bow_kf_f
        check(fn(C.byref(A), C.byref(B), C.c_float(self.mfNNratio), int(self.mbCheckOrientation), ptr(match),
                 C.byref(n), self.device), "orbx_search_by_bow")
        return match, n.value

    def SearchByProjection(self, F, vpMapPoints, th=3.0, frustum=False, viewingCosLimit=0.5):
        """SearchByProjection(Frame&, const vector<MapPoint*>&, th) -- src/ORBmatcher.cc:46-142.

        F: frame dict (synth.projection_frame layout); vpMapPoints: points dict with the track
        fields (track = mTrackProjX/Y/XR/ViewCos, track_level) or, with frustum=True, the
        isInFrustum inputs (pos, normal, dist_minmax) of Tracking::SearchLocalPoints.  Returns
        (nmatches, frame_out, point_match[, track, track_level]); frame_out[i] = point now held by
        feature i, -1 unchanged."""
        o = _run_projection(self, F, vpMapPoints, PROJ_LOCAL, th=th, frustum=frustum,
                            view_cos_limit=viewingCosLimit)
        res = (int(o["nmatches"][0]), o["frame_out"], o["point_match"])
        return res + ((o["track"], o["track_level"]) if frustum else ())

    def SearchByProjectionLastFrame(self, CurrentFrame, LastFramePoints, LastTcw, th, bMono):
        """SearchByProjection(Frame&, const Frame&, th, bMono) -- src/ORBmatcher.cc:1489-1646.
        LastFramePoints: the last frame's MapPoints (pos, desc, octave, angle, flags bit0 =
        pMP && !mvbOutlier, bit1 = Observations() > 0).  frame_out[i] = -2 where the rotation
        check reset the feature to NULL."""
        o = _run_projection(self, CurrentFrame, LastFramePoints, PROJ_LAST_FRAME, th=th, mono=bMono,
                            last_Tcw=LastTcw)
        return int(o["nmatches"][0]), o["frame_out"], o["point_match"]

    def SearchByProjectionKeyFrame(self, CurrentFrame, KFPoints, th, ORBdist):
        """SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>& sAlreadyFound, th, ORBdist) --
        src/ORBmatcher.cc:1648-1795.  KFPoints flags bit0 = pMP && !isBad() && not already found."""
        o = _run_projection(self, CurrentFrame, KFPoints, PROJ_KEYFRAME, th=th, orb_dist=ORBdist)
        return int(o["nmatches"][0]), o["frame_out"], o["point_match"]

    def Fuse(self, pKF, vpMapPoints, th=3.0):
        """The matching half of Fuse(KeyFrame*, const vector<MapPoint*>&, th) --
        src/ORBmatcher.cc:944-1054.  pKF: frame dict of the KeyFrame (bounds = its int mnMinX..);
        vpMapPoints: points dict (pos, normal, dist_minmax, desc, flags bit0 = pMP && !isBad() &&
        !IsInKeyFrame(pKF)).  Returns (nFused, bestIdx[n_points] (-1 = no fuse)); the caller applies
        Replace / AddObservation in point order (:1057-1086)."""
        o = _run_projection(self, pKF, vpMapPoints, PROJ_FUSE, th=th)
        return int(o["nmatches"][0]), o["point_match"]

    def SearchByProjectionSim3(self, pKF, Scw, vpPoints, th=10):
        """SearchByProjection(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, vector<MapPoint*>&
        vpMatched, th) -- src/ORBmatcher.cc:327-440 (LoopClosing::ComputeSim3, src/LoopClosing.cc:504).
        pKF: frame dict of the KeyFrame (bounds = its int mnMinX.., occ[i] != 0 = vpMatched[i] on
        entry); Scw: 4x4 Sim3; vpPoints: points dict (pos, normal, dist_minmax, desc, flags bit0 =
        !isBad() && not already in vpMatched).  Returns (nmatches, frame_out, point_match);
        frame_out[i] = k: vpMatched[i] = point k, -1 unchanged."""
        F = dict(pKF)
        F["Tcw"] = np.asarray(Scw, np.float32).reshape(4, 4)
        o = _run_projection(self, F, vpPoints, PROJ_SIM3, th=float(th))
        return int(o["nmatches"][0]), o["frame_out"], o["point_match"]

    def FuseSim3(self, pKF, Scw, vpPoints, th=4.0):
        """The matching half of Fuse(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, th,
        vector<MapPoint*>& vpReplacePoint) -- src/ORBmatcher.cc:1094-1236 (LoopClosing::SearchAndFuse).
        vpPoints flags bit0 = !isBad() && not in pKF->GetMapPoints().  Returns (nFused,
        bestIdx[n_points] (-1 = none)); the caller applies the replace / AddMapPoint block
        (:1210-1229) in point order."""
        F = dict(pKF)
        F["Tcw"] = np.asarray(Scw, np.float32).reshape(4, 4)
        o = _run_projection(self, F, vpPoints, PROJ_FUSE_SIM3, th=float(th))
        return int(o["nmatches"][0]), o["point_match"]

    def SearchForInitialization(self, F1, F2, vbPrevMatched, windowSize=10):
        """SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched,
        vector<int>& vnMatches12, windowSize) -- src/ORBmatcher.cc:442-587 (Tracking::
        MonocularInitialization: ORBmatcher(0.9, true), windowSize 100).  F1, F2: frame dicts
        (keys_un, desc; F2's grid fields).  Returns (nmatches, vnMatches12[N1], vbPrevMatched[N1, 2]
        updated)."""
        f1, k1 = _host_proj_frame(F1)
        f2, k2 = _host_proj_frame(F2)
        p = _lib.InitProblem()
        p.f1, p.f2 = f1, f2
        prev = np.ascontiguousarray(vbPrevMatched, np.float32).reshape(-1, 2).copy()
        assert len(prev) == f1.n
        m = np.zeros(max(1, f1.n), np.int32)
        nm = np.zeros(1, np.int32)
        p.prev_matched, p.window = ptr(prev), int(windowSize)
        p.nnratio, p.check_ori = float(self.mfNNratio), int(bool(self.mbCheckOrientation))
        p.match12, p.nmatches = ptr(m), ptr(nm)
        check(_lib.lib().orbx_search_for_initialization(C.byref(p), self.device), "orbx_search_for_initialization")
        return int(nm[0]), m[:f1.n], prev

    def SearchBySim3(self, pKF1, pKF2, pts1, pts2, s12, R12, t12, th=7.5):
        """SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, s12, R12, t12, th)
        -- src/ORBmatcher.cc:1238-1487 (LoopClosing::ComputeSim3).  pKFj: frame dicts (Tcw = GetPose());
        ptsj: the KeyFrame's GetMapPointMatches() as per-feature arrays (desc, pos, dist_minmax, flags bit0
        = pMP && !vbAlreadyMatched && !isBad()).  Returns (nFound, match12[N1]: the KF2 feature whose
        MapPoint becomes vpMatches12[i1], -1 none)."""
        f1, k1 = _host_proj_frame(pKF1)
        f2, k2 = _host_proj_frame(pKF2)
        p = _lib.Sim3Problem()
        p.kf1, p.kf2 = f1, f2
        keep = [k1, k2]
        for j, pts in ((1, pts1), (2, pts2)):
            for k, dt in (("desc", np.uint8), ("pos", np.float32), ("dist_minmax", np.float32), ("flags", np.uint8)):
                a = np.ascontiguousarray(pts[k], dt)
                keep.append(a)
                setattr(p, "%s%d" % (k, j), ptr(a))
        p.s12, p.th = float(s12), float(th)
        p.R12[:] = _f32(R12).reshape(9).tolist()
        p.t12[:] = _f32(t12).reshape(3).tolist()
        m = np.zeros(max(1, f1.n), np.int32)
        nf = np.zeros(1, np.int32)
        p.match12, p.nfound = ptr(m), ptr(nf)
        check(_lib.lib().orbx_search_by_sim3(C.byref(p), self.device), "orbx_search_by_sim3")
        return int(nf[0]), m[:f1.n]

    def SearchForTriangulation(self, prob, bOnlyStereo=False):
        """SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) --
        src/ORBmatcher.cc:738-925.  prob: dict(kf1, kf2 (keys_un, desc, u_right, has_mp, node_id,
        node_off, feat), F12[3,3], C1w[3], T2w[4,4], fx, fy, cx, cy (pKF2), scale_factors2,
        level_sigma2_2).  Returns (nmatches, vMatchedPairs as an [m,2] int array)."""
        p, keep = tri_problem(prob, bOnlyStereo, self.mbCheckOrientation)
        m12 = np.zeros(max(1, p.kf1.n), np.int32)
        nm = np.zeros(1, np.int32)
        p.match12, p.nmatches = ptr(m12), ptr(nm)
        check(_lib.lib().orbx_search_for_triangulation(C.byref(p), self.device), "orbx_search_for_triangulation")
        m12 = m12[:p.kf1.n]
        i = np.nonzero(m12 >= 0)[0]
        return int(nm[0]), np.stack([i, m12[i]], 1).astype(np.int64)

    @staticmethod
    def DescriptorDistance(a, b):
        """Hamming distance of 32-byte descriptors; a, b: [32] or [n,32] uint8 (computed on the GPU)."""
        import torch
        a = np.atleast_2d(np.ascontiguousarray(a, np.uint8))
        b = np.atleast_2d(np.ascontiguousarray(b, np.uint8))
        assert a.shape == b.shape and a.shape[1] == 32
        n = a.shape[0]
        da = torch.from_numpy(a).cuda()
        db = torch.from_numpy(b).cuda()
        out = torch.empty(n, dtype=torch.int32, device=da.device)
        s = torch.cuda.current_stream()
        check(_lib.lib().orbx_descriptor_distance_device(ptr(da), ptr(db), n, ptr(out), _stream_ptr(s)),
              "orbx_descriptor_distance_device")
        d = out.cpu().numpy()
        return int(d[0]) if n == 1 else d


PROJ_LOCAL, PROJ_LAST_FRAME, PROJ_KEYFRAME, PROJ_FUSE, PROJ_SIM3, PROJ_FUSE_SIM3 = 0, 1, 2, 3, 4, 5


def _f32(x):
    return np.ascontiguousarray(x, np.float32)


def proj_problem(frame, points, kind, th, nnratio=0.6, check_ori=True, mono=False, orb_dist=100, last_Tcw=None,
                 frustum=False, view_cos_limit=0.5, outputs=None):
    """Fill an orbx_proj_problem from a frame dict and a points dict (synth.projection_frame /
    projection_points layout).  Arrays may be host numpy arrays (for orbx_search_by_projection) or
    device tensors (for orbx_search_by_projection_device); the caller keeps them alive.  `outputs`
    = dict(frame_out, point_match, nmatches[, track, track_level]); numpy arrays are allocated when
    absent.  Returns (problem, outputs)."""
    n, npnt = len(frame["desc"]), len(points["desc"])
    if outputs is None:
        outputs = dict(frame_out=np.zeros(n, np.int32), point_match=np.zeros(npnt, np.int32),
                       nmatches=np.zeros(1, np.int32))
        if kind == PROJ_LOCAL:
            outputs["track"] = (np.zeros((npnt, 4), np.float32) if frustum
                                else np.ascontiguousarray(points["track"], np.float32))
            outputs["track_level"] = (np.zeros(npnt, np.int32) if frustum
                                      else np.ascontiguousarray(points["track_level"], np.int32))
    f = _lib.ProjFrame()
    f.n = n
    f.keys_un, f.desc = ptr(frame["keys_un"]), ptr(frame["desc"])
    f.u_right = ptr(frame.get("u_right"))
    f.occ = ptr(frame.get("occ"))
    for k in ("min_x", "max_x", "min_y", "max_y", "grid_inv_w", "grid_inv_h", "log_scale_factor", "fx", "fy",
              "cx", "cy", "bf", "b"):
        setattr(f, k, float(frame[k]))
    if frame.get("grid_min_x") is not None:  # a KeyFrame's grid: the Frame's float bounds
        f.grid_min_x, f.grid_min_y, f.grid_min_set = float(frame["grid_min_x"]), float(frame["grid_min_y"]), 1
    f.nlevels = int(frame["nlevels"])
    sf = np.zeros(16, np.float32)
    sf[:f.nlevels] = frame["scale_factors"][:f.nlevels]
    f.scale_factors[:] = sf.tolist()
    isg = np.zeros(16, np.float32)
    if frame.get("inv_level_sigma2") is not None:
        isg[:f.nlevels] = frame["inv_level_sigma2"][:f.nlevels]
    else:  # mvInvLevelSigma2 = 1 / (s*s) in float (ORBextractor ctor)
        isg[:f.nlevels] = np.float32(1.0) / (sf[:f.nlevels] * sf[:f.nlevels])
    f.inv_level_sigma2[:] = isg.tolist()
    f.Tcw[:] = _f32(frame["Tcw"]).reshape(16).tolist()
    p = _lib.ProjProblem()
    p.kind, p.frustum, p.f, p.n_points = int(kind), int(bool(frustum)), f, npnt
    p.desc, p.flags = ptr(points["desc"]), ptr(points["flags"])
    for k in ("pos", "normal", "dist_minmax", "angle", "octave"):
        setattr(p, k, ptr(points.get(k)))
    p.track = ptr(outputs.get("track"))
    p.track_level = ptr(outputs.get("track_level"))
    p.th, p.nnratio, p.view_cos_limit = float(th), float(nnratio), float(view_cos_limit)
    p.check_ori, p.mono, p.orb_dist = int(bool(check_ori)), int(bool(mono)), int(orb_dist)
    p.last_Tcw[:] = (_f32(last_Tcw).reshape(16) if last_Tcw is not None else np.eye(4, dtype=np.float32).reshape(16)).tolist()
    p.frame_out, p.point_match, p.nmatches = (ptr(outputs["frame_out"]), ptr(outputs["point_match"]),
                                              ptr(outputs["nmatches"]))
    return p, outputs


def _host_proj_frame(frame):
    """An orbx_proj_frame over host copies of a frame dict's arrays; returns (frame, keep-alive)."""
    fr = _host_frame(frame)
    p, _ = proj_problem(fr, dict(desc=np.zeros((0, 32), np.uint8), flags=np.zeros(0, np.uint8)), PROJ_KEYFRAME,
                        th=1.0, outputs=dict(frame_out=None, point_match=None, nmatches=None))
    return p.f, fr


def _host_points(points):
    out = dict(points)
    for k, dt in (("desc", np.uint8), ("flags", np.uint8), ("pos", np.float32), ("normal", np.float32),
                  ("dist_minmax", np.float32), ("angle", np.float32), ("octave", np.int32)):
        if points.get(k) is not None:
            out[k] = np.ascontiguousarray(points[k], dt)
    return out


def _host_frame(frame):
    out = dict(frame)
    out["keys_un"] = np.ascontiguousarray(frame["keys_un"], KEYPOINT_DTYPE)
    out["desc"] = np.ascontiguousarray(frame["desc"], np.uint8)
    if frame.get("u_right") is not None:
        out["u_right"] = np.ascontiguousarray(frame["u_right"], np.float32)
    if frame.get("occ") is not None:
        out["occ"] = np.ascontiguousarray(frame["occ"], np.int8)
    return out


def _run_projection(matcher, frame, points, kind, **kw):
    fr, pts = _host_frame(frame), _host_points(points)
    p, out = proj_problem(fr, pts, kind, nnratio=matcher.mfNNratio, check_ori=matcher.mbCheckOrientation, **kw)
    check(_lib.lib().orbx_search_by_projection(C.byref(p), matcher.device), "orbx_search_by_projection")
    return out


def tri_problem(prob, only_stereo=False, check_ori=True):
    """orbx_tri_problem from a dict whose arrays are host numpy arrays or device tensors (the caller
    keeps them alive; numpy inputs are made contiguous here and returned in `keep`).  match12 and
    nmatches are left for the caller to point at its outputs."""
    keep = []

    def arr(x, dt):
        if x is None or not isinstance(x, np.ndarray):
            return x
        a = np.ascontiguousarray(x, dt)
        keep.append(a)
        return a

    def kf(d):
        k = _lib.TriKF()
        keys = arr(d["keys_un"], KEYPOINT_DTYPE)
        k.n = len(d["desc"])
        k.keys_un, k.desc = ptr(keys), ptr(arr(d["desc"], np.uint8))
        k.u_right, k.has_mp = ptr(arr(d.get("u_right"), np.float32)), ptr(arr(d.get("has_mp"), np.uint8))
        k.n_nodes = len(d["node_id"])
        k.node_id, k.node_off = ptr(arr(d["node_id"], np.uint32)), ptr(arr(d["node_off"], np.int32))
        k.feat = ptr(arr(d["feat"], np.int32))
        return k

    p = _lib.TriProblem()
    p.kf1, p.kf2 = kf(prob["kf1"]), kf(prob["kf2"])
    p.F12[:] = _f32(prob["F12"]).reshape(9).tolist()
    p.C1w[:] = _f32(prob["C1w"]).reshape(3).tolist()
    p.T2w[:] = _f32(prob["T2w"]).reshape(16).tolist()
    for k in ("fx", "fy", "cx", "cy"):
        setattr(p, k, float(prob[k]))
    sf = np.zeros(16, np.float32)
    sg = np.zeros(16, np.float32)
    nl = len(prob["scale_factors2"])
    sf[:nl], sg[:nl] = prob["scale_factors2"], prob["level_sigma2_2"]
    p.scale_factors2[:] = sf.tolist()
    p.level_sigma2_2[:] = sg.tolist()
    p.only_stereo, p.check_ori = int(bool(only_stereo)), int(bool(check_ori))
    return p, keep


def _ba_arrays(prob):
    """Problem dict -> contiguous arrays in the orbx_ba_problem layout."""
    nc = len(prob["Tcw"])
    fixed = prob.get("fixed")
    return dict(Tcw=np.ascontiguousarray(np.asarray(prob["Tcw"], np.float32).reshape(nc, 12)),
                fixed=np.ascontiguousarray(np.zeros(nc, np.uint8) if fixed is None else fixed, np.uint8),
                intr=np.ascontiguousarray(np.asarray(prob["intr"], np.float32).reshape(nc, 5)),
                Xw=np.ascontiguousarray(np.asarray(prob["Xw"], np.float32).reshape(-1, 3)),
                edge_point=np.ascontiguousarray(prob["edge_point"], np.int32),
                edge_cam=np.ascontiguousarray(prob["edge_cam"], np.int32),
                obs=np.ascontiguousarray(np.asarray(prob["obs"], np.float32).reshape(-1, 3)),
                inv_sigma2=np.ascontiguousarray(prob["inv_sigma2"], np.float32))


class Optimizer:
    """Optimizer::LocalBundleAdjustment (include/Optimizer.h:46) on the GPU.

    The solver handle keeps device buffers between calls (the local mapping
    thread runs one LocalBA per new keyframe)."""

    def __init__(self, device=0, priority=0, cu_mask=None):
        """priority: HIP stream priority of the handle's stream (0 default, < 0 higher; see
        orbx_ba_create_priority) -- the LocalMapping thread's handle runs high beside extraction.
        cu_mask: optional sequence of 32-bit words restricting the handle's stream to a CU set
        (orbx_ba_create_masked; the priority is then the default)."""
        h = C.c_void_p()
        if cu_mask is not None:
            m = np.ascontiguousarray(cu_mask, np.uint32)
            check(_lib.lib().orbx_ba_create_masked(int(device), ptr(m), len(m), C.byref(h)), "orbx_ba_create_masked")
        else:
            check(_lib.lib().orbx_ba_create_priority(int(device), int(priority), C.byref(h)), "orbx_ba_create_priority")
        self._h = h
        self.device = int(device)
        f = C.POINTER(C.c_int)()
        check(_lib.lib().orbx_ba_stop_flag(h, C.byref(f)), "orbx_ba_stop_flag")
        self._stop = f  # the handle's pinned flag (the device polls it without registration)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().orbx_ba_destroy(self._h)
            self._h = None
            self._stop = None

    def set_debug_options(self, **kw):
        """Test options of this solver handle (include/orbx_debug.h, orbx_ba_debug_options: ldlt,
        nan_trial, raise_stop_after, trace, fused_ctl); no arguments restore the production defaults."""
        o = _lib.BaDebugOptions(0, -1, -1, 0)
        for k, v in kw.items():
            if k not in dict(o._fields_):
                raise TypeError("unknown LocalBA debug option %r" % k)
            setattr(o, k, int(v))
        check(_lib.lib().orbx_debug_ba_options(self._h, C.byref(o)), "orbx_debug_ba_options")

    @contextlib.contextmanager
    def debug_options(self, **kw):
        self.set_debug_options(**kw)
        try:
            yield self
        finally:
            self.set_debug_options()

    def capture_select(self, phase, it=-1, q=0):
        """Record one LM trial of the next LocalBundleAdjustment call (include/orbx_debug.h,
        orbx_debug_ba_capture_select; tests only): the first trial of `phase` (0 / 1) at iteration
        `it` of the phase (-1: any) with trial index `q` inside its iteration.  phase < 0 disarms."""
        check(_lib.lib().orbx_debug_ba_capture_select(self._h, int(phase), int(it), int(q)),
              "orbx_debug_ba_capture_select")

    def capture_read(self):
        """The last capture as a dict (orbx_debug_ba_capture_read), or None when none fired: the header
        fields (_lib.BA_CAPTURE_HEADER), `lambda`, `chi`, and every item of _lib.BA_CAPTURE_ITEMS; the
        linearised state is composed as cq_lin / ct_lin / X_lin (cbak / Xbak over the current state)."""
        L = _lib.lib()
        hdr = np.zeros(len(_lib.BA_CAPTURE_HEADER), np.int32)
        n = L.orbx_debug_ba_capture_read(self._h, 0, ptr(hdr), hdr.nbytes)
        if n != hdr.nbytes:
            raise _lib.OrbxError(int(n), "orbx_debug_ba_capture_read")
        c = dict(zip(_lib.BA_CAPTURE_HEADER, (int(v) for v in hdr)))
        if not c["fired"]:
            return None
        for name, (what, dt, tail) in _lib.BA_CAPTURE_ITEMS.items():
            n = L.orbx_debug_ba_capture_read(self._h, what, None, 0)
            if n < 0:
                raise _lib.OrbxError(int(n), "orbx_debug_ba_capture_read")
            a = np.zeros(n // np.dtype(dt).itemsize, dt)
            if n:
                L.orbx_debug_ba_capture_read(self._h, what, ptr(a), a.nbytes)
            c[name] = a.reshape((-1,) + tail)
        N = 6 * c["nposes"]
        c["S"] = c["S"].reshape(N, N)
        c["lambda"], c["chi"] = (float(v) for v in c.pop("lambda_chi"))
        c["cq_lin"], c["ct_lin"], c["X_lin"] = c["cq"].copy(), c["ct"].copy(), c["X"].copy()
        if c["ok"]:
            c["cq_lin"][c["pose_cam"]] = c["cbak"][:, :4]
            c["ct_lin"][c["pose_cam"]] = c["cbak"][:, 4:]
            c["X_lin"][c["pt_id"]] = c["Xbak"]
        return c

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def PoseOptimization(self, frame):
        """Optimizer::PoseOptimization(Frame*) -- src/Optimizer.cc:287-528.  frame: dict(obs[n,3]
        (u, v, ur; ur < 0 = monocular), Xw[n,3], inv_sigma2[n], fx, fy, cx, cy, bf, Tcw[4,4]) with
        one row per feature that has a MapPoint, in feature order.  Returns (nGood, Tcw[4,4],
        outlier[n] (mvbOutlier), iterations[4])."""
        pr = dict(frame)
        pr["obs"] = np.ascontiguousarray(frame["obs"], np.float32).reshape(-1, 3)
        pr["Xw"] = np.ascontiguousarray(frame["Xw"], np.float32).reshape(-1, 3)
        pr["inv_sigma2"] = np.ascontiguousarray(frame["inv_sigma2"], np.float32)
        p, out = pose_problem_struct(pr)
        check(_lib.lib().orbx_pose_optimization(C.byref(p), self.device), "orbx_pose_optimization")
        return int(out["ngood"][0]), out["Tcw_out"], out["outlier"][:len(pr["obs"])], out["iterations"]

    def OptimizeSim3(self, problem):
        """Optimizer::OptimizeSim3 -- src/Optimizer.cc:1220-1456.  problem: dict(x3dc1[n,3], x3dc2[n,3]
        (camera-frame points of the correspondences the intake loop keeps, in its order), obs1[n,2],
        obs2[n,2], inv_sigma2_1[n], inv_sigma2_2[n], K1, K2 (fx, fy, cx, cy), S12 (8 doubles: quaternion
        x, y, z, w, translation, scale), th2, bFixScale).  Returns (nIn, S12[8], inlier[n] (0 where the
        reference nulls vpMatches1), n_bad, iterations[2], trials)."""
        pr = dict(problem)
        for k, w in (("x3dc1", 3), ("x3dc2", 3), ("obs1", 2), ("obs2", 2)):
            pr[k] = np.ascontiguousarray(problem[k], np.float32).reshape(-1, w)
        for k in ("inv_sigma2_1", "inv_sigma2_2"):
            pr[k] = np.ascontiguousarray(problem[k], np.float32).reshape(-1)
        p, out = optimize_sim3_problem_struct(pr)
        check(_lib.lib().orbx_optimize_sim3(C.byref(p), self.device), "orbx_optimize_sim3")
        return (int(out["n_in"][0]), out["S12_out"], out["inlier"][:len(pr["x3dc1"])], int(out["n_bad"][0]),
                out["iterations"], int(out["trials"][0]))

    def OptimizeEssentialGraph(self, M):
        """Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
        LoopConnections, bFixScale) -- src/Optimizer.cc:888-1218.  M, the map: dict(keyframes = [dict(id,
        Tcw[3,4] float32, parent (an id or None), children (set of ids), loop_edges (set of ids),
        covisibles ([(id, weight)] in GetVectorCovisibleKeyFrames' order, weights descending), bad)],
        pLoopKF, pCurKF (ids), NonCorrectedSim3, CorrectedSim3 ({id: 8 doubles, quaternion x, y, z, w,
        translation, scale}), LoopConnections ({id: set of ids}), bFixScale, points = [dict(pos[3] float32,
        mnCorrectedByKF, mnCorrectedReference, ref (the reference keyframe's id), bad)]).

        The edge selection (:981-1138) is the reference's: the minFeat = 100 rule and its exception for the
        (pCurKF, pLoopKF) pair, sInsertedEdges, the mnId ordering tests, GetCovisiblesByWeight(100), the
        pParentKF / hasChild / sLoopEdges exclusions.  The reference walks its std::map<KeyFrame*, ...> and
        std::set<KeyFrame*> in pointer order, which no run reproduces: here keyframes are walked in
        ASCENDING ID (edge order changes summation order only).  A bad keyframe gets no vertex, edges that
        would touch it are not added (g2o refuses an edge with a null vertex) and its pose stays.

        Returns dict(Tcw {id: [3,4] float32, what SetPose receives}, pos {point index: [3] float32, what
        SetWorldPos receives}, Scw {id: 8 doubles, the optimised Sim3}, edges [(nIDi, nIDj, kind)],
        iterations, trials, chi2_initial, chi2_final, solver_failures)."""
        P, ids, pts, edges = essential_graph_problem(M)
        p, r, out = essential_graph_structs(P)
        check(_lib.lib().orbx_optimize_essential_graph(C.byref(p), C.byref(r), self.device),
              "orbx_optimize_essential_graph")
        return dict(Tcw={i: out["Tcw_out"][k].reshape(3, 4) for k, i in enumerate(ids)},
                    pos={k: out["Xw_out"][j] for j, k in enumerate(pts)},
                    Scw={i: out["Scw_out"][k] for k, i in enumerate(ids)}, edges=edges,
                    iterations=int(out["iterations"][0]), trials=int(out["trials"][0]),
                    chi2_initial=float(out["chi2_initial"][0]), chi2_final=float(out["chi2_final"][0]),
                    solver_failures=int(out["solver_failures"][0]), raw=out, problem=P)

    def LocalBundleAdjustment(self, prob, stop=False):
        """prob: dict(Tcw[n,12], fixed[n], intr[n,5] fx,fy,cx,cy,bf, Xw[m,3], edge_point, edge_cam,
        obs[e,3] (u, v, ur; ur<0 mono), inv_sigma2[e]).  ``stop`` mirrors *pbStopFlag: a bool, or
        a one-element int32 array another thread may set while the call runs (the LM loop polls
        it between iterations and trials, src/Optimizer.cc:749-762).

        Returns dict(Tcw, Xw, edge_outlier, Tcw_d, Xw_d, iterations, trials, chi2)."""
        a = _ba_arrays(prob)
        nc, npt, ne = len(a["Tcw"]), len(a["Xw"]), len(a["edge_point"])
        P = _lib.BaProblem(nc, ptr(a["Tcw"]), ptr(a["fixed"]), ptr(a["intr"]), npt, ptr(a["Xw"]), ne,
                           ptr(a["edge_point"]), ptr(a["edge_cam"]), ptr(a["obs"]), ptr(a["inv_sigma2"]))
        # (every output element is written by the call: no zero fill)
        out = dict(Tcw=np.empty((nc, 12), np.float32), Xw=np.empty((npt, 3), np.float32),
                   edge_outlier=np.empty(ne, np.uint8), Tcw_d=np.empty((nc, 12)), Xw_d=np.empty((npt, 3)))
        R = _lib.BaResult(ptr(out["Tcw"]), ptr(out["Xw"]), ptr(out["edge_outlier"]), ptr(out["Tcw_d"]),
                          ptr(out["Xw_d"]))
        if isinstance(stop, np.ndarray):
            if stop.dtype != np.int32 or stop.size != 1 or not stop.flags.c_contiguous:
                raise ValueError("stop flag array must be one contiguous int32")
            flag = C.c_void_p(stop.ctypes.data)
        else:
            self._stop[0] = 1 if stop else 0
            flag = C.cast(self._stop, C.c_void_p)
        check(_lib.lib().orbx_ba_run(self._h, C.byref(P), C.byref(R), flag), "orbx_ba_run")
        out.update(iterations=tuple(R.iterations), trials=R.trials, chi2=tuple(R.chi2))
        return out

    def GlobalBundleAdjustemnt(self, problem, nIterations=5, stop=False, bRobust=True):
        """Optimizer::GlobalBundleAdjustemnt -> BundleAdjustment (src/Optimizer.cc:41-284; the reference's
        spelling): one optimize(nIterations) over every edge of ``problem`` (LocalBundleAdjustment's
        dict: cameras fixed for mnId == 0, edges per point in point order), Huber kernels with the
        deltas sqrt(5.99) / sqrt(7.815) when bRobust, none otherwise.  ``stop`` as in
        LocalBundleAdjustment; a flag raised before the call gives zero iterations and the outputs
        are the inputs through toSE3Quat / toCvMat (there is no early return).  Up to 512 free
        keyframes (OrbxError ORBX_ERR_SIZE beyond).

        Returns LocalBundleAdjustment's dict (edge_outlier all zero, iterations[1] = chi2[1] = 0)
        plus point_included[m] (0: the point had no edge and keeps its position) and ran (1)."""
        a = _ba_arrays(problem)
        nc, npt, ne = len(a["Tcw"]), len(a["Xw"]), len(a["edge_point"])
        P = _lib.BaProblem(nc, ptr(a["Tcw"]), ptr(a["fixed"]), ptr(a["intr"]), npt, ptr(a["Xw"]), ne,
                           ptr(a["edge_point"]), ptr(a["edge_cam"]), ptr(a["obs"]), ptr(a["inv_sigma2"]))
        out = dict(Tcw=np.empty((nc, 12), np.float32), Xw=np.empty((npt, 3), np.float32),
                   edge_outlier=np.zeros(ne, np.uint8), Tcw_d=np.empty((nc, 12)), Xw_d=np.empty((npt, 3)),
                   point_included=np.zeros(npt, np.uint8))
        R = _lib.BaResult(ptr(out["Tcw"]), ptr(out["Xw"]), ptr(out["edge_outlier"]), ptr(out["Tcw_d"]),
                          ptr(out["Xw_d"]))
        if isinstance(stop, np.ndarray):
            if stop.dtype != np.int32 or stop.size != 1 or not stop.flags.c_contiguous:
                raise ValueError("stop flag array must be one contiguous int32")
            flag = C.c_void_p(stop.ctypes.data)
        else:
            self._stop[0] = 1 if stop else 0
            flag = C.cast(self._stop, C.c_void_p)
        check(_lib.lib().orbx_ba_run_global(self._h, C.byref(P), int(nIterations), 1 if bRobust else 0, C.byref(R),
                                            ptr(out["point_included"]), flag), "orbx_ba_run_global")
        out.update(iterations=tuple(R.iterations), trials=R.trials, chi2=tuple(R.chi2), ran=R.ran)
        return out

    def LocalBundleAdjustmentMany(self, probs, stop=False):
        """K independent problems through one batched LM loop (orbx_ba_run_many); returns the
        list of result dicts, each bit-identical to LocalBundleAdjustment on that problem."""
        K = len(probs)
        keep, outs = [], []
        Ps, Rs = (_lib.BaProblem * K)(), (_lib.BaResult * K)()
        for k, prob in enumerate(probs):
            a = _ba_arrays(prob)
            nc, npt, ne = len(a["Tcw"]), len(a["Xw"]), len(a["edge_point"])
            Ps[k] = _lib.BaProblem(nc, ptr(a["Tcw"]), ptr(a["fixed"]), ptr(a["intr"]), npt, ptr(a["Xw"]), ne,
                                   ptr(a["edge_point"]), ptr(a["edge_cam"]), ptr(a["obs"]), ptr(a["inv_sigma2"]))
            out = dict(Tcw=np.empty((nc, 12), np.float32), Xw=np.empty((npt, 3), np.float32),
                       edge_outlier=np.empty(ne, np.uint8), Tcw_d=np.empty((nc, 12)), Xw_d=np.empty((npt, 3)))
            Rs[k] = _lib.BaResult(ptr(out["Tcw"]), ptr(out["Xw"]), ptr(out["edge_outlier"]), ptr(out["Tcw_d"]),
                                  ptr(out["Xw_d"]))
            keep.append(a)
            outs.append(out)
        self._stop[0] = 1 if stop else 0
        check(_lib.lib().orbx_ba_run_many(self._h, K, Ps, Rs, C.cast(self._stop, C.c_void_p)), "orbx_ba_run_many")
        for k in range(K):
            outs[k].update(iterations=tuple(Rs[k].iterations), trials=Rs[k].trials, chi2=tuple(Rs[k].chi2))
        return outs


def pose_problem_struct(prob, outputs=None):
    """orbx_pose_problem from a dict (host numpy or device tensors); outputs allocated on the host
    when absent.  Returns (struct, outputs)."""
    n = len(prob["obs"])
    if outputs is None:
        outputs = dict(Tcw_out=np.zeros((4, 4), np.float32), outlier=np.zeros(max(n, 1), np.uint8),
                       ngood=np.zeros(1, np.int32), iterations=np.zeros(4, np.int32))
    p = _lib.PoseProblem()
    p.n = n
    p.obs, p.Xw, p.inv_sigma2 = ptr(prob["obs"]), ptr(prob["Xw"]), ptr(prob["inv_sigma2"])
    for k in ("fx", "fy", "cx", "cy", "bf"):
        setattr(p, k, float(prob[k]))
    p.Tcw[:] = _f32(prob["Tcw"]).reshape(16).tolist()
    p.Tcw_out, p.outlier, p.ngood = ptr(outputs["Tcw_out"]), ptr(outputs["outlier"]), ptr(outputs["ngood"])
    p.iterations = ptr(outputs.get("iterations"))
    return p, outputs


def essential_graph_edges(M):
    """The edges Optimizer::OptimizeEssentialGraph adds (src/Optimizer.cc:981-1138), keyframes walked in
    ascending id: [(nIDi, nIDj, kind)] in insertion order, kind 0 = a LoopConnections edge (measured from
    vScw), 1 = a spanning-tree, old-loop or covisibility edge (measured from NonCorrectedSim3)."""
    minFeat = 100
    kfs = {kf["id"]: kf for kf in M["keyframes"]}
    is_vertex = {i: not kf["bad"] for i, kf in kfs.items()}
    nCur, nLoop = M["pCurKF"], M["pLoopKF"]
    edges, sInsertedEdges = [], set()

    def GetWeight(kf, j):  # KeyFrame::GetWeight (src/KeyFrame.cc:265-272)
        for i, w in kf["covisibles"]:
            if i == j:
                return w
        return 0
    # Set Loop edges (:981-1019)
    for nIDi in sorted(M["LoopConnections"]):
        pKF = kfs[nIDi]
        for nIDj in sorted(M["LoopConnections"][nIDi]):
            if (nIDi != nCur or nIDj != nLoop) and GetWeight(pKF, nIDj) < minFeat:
                continue
            if is_vertex[nIDi] and is_vertex[nIDj]:
                edges.append((nIDi, nIDj, 0))
            sInsertedEdges.add((min(nIDi, nIDj), max(nIDi, nIDj)))
    # Set normal edges (:1024-1138)
    for nIDi in sorted(kfs):
        pKF = kfs[nIDi]
        if not is_vertex[nIDi]:
            continue
        pParentKF = pKF["parent"]
        if pParentKF is not None and is_vertex[pParentKF]:  # spanning tree edge
            edges.append((nIDi, pParentKF, 1))
        sLoopEdges = set(pKF["loop_edges"])
        for nIDl in sorted(sLoopEdges):  # loop edges
            if nIDl < nIDi and is_vertex[nIDl]:
                edges.append((nIDi, nIDl, 1))
        # GetCovisiblesByWeight(minFeat) (src/KeyFrame.cc:239-255): the ordered list up to the first weight
        # below minFeat -- and, as the reference has it, NOTHING when no weight is below it (upper_bound
        # reaches end())
        cut = next((k for k, (_, w) in enumerate(pKF["covisibles"]) if w < minFeat), 0)
        for nIDn, w in pKF["covisibles"][:cut]:
            if nIDn != pParentKF and nIDn not in pKF["children"] and nIDn not in sLoopEdges:
                if not kfs[nIDn]["bad"] and nIDn < nIDi:
                    if (min(nIDi, nIDn), max(nIDi, nIDn)) in sInsertedEdges:
                        continue
                    edges.append((nIDi, nIDn, 1))
    return edges


def essential_graph_problem(M):
    """The map description of Optimizer.OptimizeEssentialGraph -> (problem dict of host arrays, the vertices'
    keyframe ids, the indices of the points the call moves, the edges as ids)."""
    kfs = sorted((kf for kf in M["keyframes"] if not kf["bad"]), key=lambda kf: kf["id"])
    ids = [kf["id"] for kf in kfs]
    index = {i: k for k, i in enumerate(ids)}
    n = len(ids)
    Scw, Snc = np.zeros((n, 8)), np.zeros((n, 8))
    for k, kf in enumerate(kfs):
        if kf["id"] in M["CorrectedSim3"]:
            Scw[k] = np.asarray(M["CorrectedSim3"][kf["id"]], np.float64)
        else:
            T = np.ascontiguousarray(np.asarray(kf["Tcw"], np.float32).reshape(-1)[:12])
            _lib.lib().orbx_sim3_from_tcw(ptr(T), ptr(Scw[k:k + 1]))
        Snc[k] = np.asarray(M["NonCorrectedSim3"][kf["id"]], np.float64) if kf["id"] in M["NonCorrectedSim3"] else Scw[k]
    edges = essential_graph_edges(M)
    pts, Xw, ref = [], [], []
    for k, mp in enumerate(M["points"]):
        if mp["bad"]:
            continue
        nIDr = mp["mnCorrectedReference"] if mp["mnCorrectedByKF"] == M["pCurKF"] else mp["ref"]
        if nIDr not in index:
            continue
        pts.append(k)
        Xw.append(np.asarray(mp["pos"], np.float32).reshape(3))
        ref.append(index[nIDr])
    P = dict(vertex_id=np.array(ids, np.int32), Scw=Scw, Snc=Snc, fixed_vertex=index[M["pLoopKF"]],
             bFixScale=bool(M["bFixScale"]), edge_v0=np.array([index[e[0]] for e in edges], np.int32),
             edge_v1=np.array([index[e[1]] for e in edges], np.int32),
             edge_kind=np.array([e[2] for e in edges], np.uint8), iterations=20, lambda_init=1e-16,
             Xw=np.array(Xw, np.float32).reshape(-1, 3), point_ref=np.array(ref, np.int32))
    return P, ids, pts, edges


def essential_graph_structs(P, outputs=None):
    """orbx_essential_graph_problem / _result from a problem dict (host numpy or device tensors; the graph's
    structure always host numpy); outputs allocated on the host when absent.  Returns (problem, result,
    outputs); the structs borrow the dict's arrays."""
    n, m = len(P["vertex_id"]), len(P["point_ref"])
    if outputs is None:
        outputs = dict(Scw_out=np.zeros((n, 8)), Tcw_out=np.zeros((n, 12), np.float32),
                       Xw_out=np.zeros((max(m, 1), 3), np.float32)[:m], iterations=np.zeros(1, np.int32),
                       trials=np.zeros(1, np.int32), chi2_initial=np.zeros(1), chi2_final=np.zeros(1),
                       solver_failures=np.zeros(1, np.int32))
    p = _lib.EssGraphProblem()
    p.n_vertices, p.n_edges, p.n_points = n, len(P["edge_v0"]), m
    for k in ("vertex_id", "Scw", "Snc", "edge_v0", "edge_v1", "edge_kind", "Xw", "point_ref"):
        setattr(p, k, ptr(P[k]))
    p.fixed_vertex = int(P["fixed_vertex"])
    p.fix_scale = 1 if P["bFixScale"] else 0
    p.iterations = int(P["iterations"])
    p.lambda_init = float(P["lambda_init"])
    r = _lib.EssGraphResult()
    for k in ("Scw_out", "Tcw_out", "Xw_out", "iterations", "trials", "chi2_initial", "chi2_final", "solver_failures"):
        setattr(r, k, ptr(outputs.get(k)))
    return p, r, outputs


def optimize_sim3_problem_struct(prob, outputs=None):
    """orbx_optimize_sim3_problem from a dict (host numpy or device tensors); outputs allocated on the
    host when absent.  Returns (struct, outputs)."""
    n = len(prob["x3dc1"])
    if outputs is None:
        outputs = dict(S12_out=np.zeros(8, np.float64), inlier=np.zeros(max(n, 1), np.uint8),
                       n_in=np.zeros(1, np.int32), n_bad=np.zeros(1, np.int32), iterations=np.zeros(2, np.int32),
                       trials=np.zeros(1, np.int32))
    p = _lib.OptSim3Problem()
    p.n = n
    for k in ("x3dc1", "x3dc2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
        setattr(p, k, ptr(prob[k]))
    p.K1[:] = _f32(prob["K1"]).reshape(4).tolist()
    p.K2[:] = _f32(prob["K2"]).reshape(4).tolist()
    p.S12[:] = np.asarray(prob["S12"], np.float64).reshape(8).tolist()
    p.th2 = float(prob["th2"])
    p.fix_scale = 1 if prob["bFixScale"] else 0
    for k in ("S12_out", "inlier", "n_in", "n_bad", "iterations", "trials"):
        setattr(p, k, ptr(outputs.get(k)))
    return p, outputs


class PnPsolver:
    """PnPsolver (include/PnPsolver.h:66-77) over orbx_pnp_*.

    Correspondences are given in the constructor's gather order
    (src/PnPsolver.cc:67-125): world points, undistorted keypoints and
    mvLevelSigma2[octave] of the matched keypoints.  Like the reference the
    constructor applies SetRansacParameters() with its defaults."""

    def __init__(self, p3d, p2d, sigma2, fx, fy, cx, cy, device=0):
        self.p3d = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
        self.p2d = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
        self.sigma2 = np.ascontiguousarray(sigma2, np.float32)
        self.n = len(self.p3d)
        self.intr = (float(fx), float(fy), float(cx), float(cy))
        self.device = int(device)
        self._h = None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4,
                            th2=5.991):
        """src/PnPsolver.cc:136-179.  May be called at any time: after iterate() the derived parameters
        and maxError are recomputed in place and the iteration count / best set are kept, as in the
        reference."""
        prm = _lib.PnpParams(float(probability), int(minInliers), int(maxIterations), int(minSet), float(epsilon),
                             float(th2))
        if self._h:
            check(_lib.lib().orbx_pnp_set_ransac_parameters(self._h, ptr(self.sigma2), C.byref(prm)),
                  "orbx_pnp_set_ransac_parameters")
            self._read_params(minSet)
            return
        prob = _lib.PnpProblem(self.n, ptr(self.p3d), ptr(self.p2d), ptr(self.sigma2), *self.intr)
        h = C.c_void_p()
        check(_lib.lib().orbx_pnp_create(C.byref(prob), C.byref(prm), self.device, C.byref(h)), "orbx_pnp_create")
        self._adopt(h, minSet)

    def _read_params(self, minSet):
        self.min_set = int(minSet)
        a, b, c = C.c_int(), C.c_int(), C.c_float()
        check(_lib.lib().orbx_pnp_get_params(self._h, C.byref(a), C.byref(b), C.byref(c)), "orbx_pnp_get_params")
        self.min_inliers, self.max_its, self.epsilon = a.value, b.value, c.value

    def _adopt(self, h, minSet):
        """Takes a fresh orbx_pnp handle: the derived parameters, no hypothesis run yet."""
        self._h = h
        self._read_params(minSet)
        self._done = 0

    @classmethod
    def create_many(cls, problems, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4,
                    th2=5.991, device=0):
        """len(problems) solvers (dicts p3d, p2d, sigma2, fx, fy, cx, cy) with one parameter set, created by
        one orbx_pnp_create_many call (one upload for all correspondences)."""
        n = len(problems)
        objs, structs = [], (_lib.PnpProblem * max(n, 1))()
        for i, P in enumerate(problems):
            o = cls.__new__(cls)
            o.p3d = np.ascontiguousarray(P["p3d"], np.float32).reshape(-1, 3)
            o.p2d = np.ascontiguousarray(P["p2d"], np.float32).reshape(-1, 2)
            o.sigma2 = np.ascontiguousarray(P["sigma2"], np.float32)
            o.n = len(o.p3d)
            o.intr = (float(P["fx"]), float(P["fy"]), float(P["cx"]), float(P["cy"]))
            o.device = int(device)
            o._h = None
            structs[i] = _lib.PnpProblem(o.n, ptr(o.p3d), ptr(o.p2d), ptr(o.sigma2), *o.intr)
            objs.append(o)
        prm = _lib.PnpParams(float(probability), int(minInliers), int(maxIterations), int(minSet), float(epsilon),
                             float(th2))
        hs = (C.c_void_p * max(n, 1))()
        check(_lib.lib().orbx_pnp_create_many(structs, n, C.byref(prm), int(device), hs), "orbx_pnp_create_many")
        for o, h in zip(objs, hs):
            o._adopt(C.c_void_p(h), minSet)
        return objs

    @classmethod
    def create_many_device(cls, p3d, p2d, sigma2, offsets, intr, probability=0.99, minInliers=8,
                           maxIterations=300, minSet=4, epsilon=0.4, th2=5.991, device=0):
        """Solvers over device-resident correspondences: p3d [M,3], p2d [M,2], sigma2 [M] float32 device
        tensors holding the problems back to back (problem i = rows offsets[i]..offsets[i+1]-1), intr [n,4]
        (fx, fy, cx, cy) on the host -- one orbx_pnp_create_many_device call."""
        offs = np.ascontiguousarray(offsets, np.int32)
        it = np.ascontiguousarray(intr, np.float32).reshape(-1, 4)
        n = len(offs) - 1
        prm = _lib.PnpParams(float(probability), int(minInliers), int(maxIterations), int(minSet), float(epsilon),
                             float(th2))
        hs = (C.c_void_p * max(n, 1))()
        check(_lib.lib().orbx_pnp_create_many_device(C.c_void_p(p3d.data_ptr()), C.c_void_p(p2d.data_ptr()),
                                                     C.c_void_p(sigma2.data_ptr()), ptr(offs), ptr(it), n,
                                                     C.byref(prm), int(device), hs), "orbx_pnp_create_many_device")
        objs = []
        for i in range(n):
            o = cls.__new__(cls)
            o.n = int(offs[i + 1] - offs[i])
            o.device = int(device)
            o._adopt(C.c_void_p(hs[i]), minSet)
            objs.append(o)
        return objs

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().orbx_pnp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def iterate(self, nIterations, rng):
        """rng: a rand() stream with peek(k)/advance(k) (e.g. glibc_rand.GlibcRand(1), the
        unseeded process rand() of the reference).  Returns (Tcw[4,4] or None, bNoMore,
        vbInliers[n] bool, nInliers); the stream advances by exactly what was drawn."""
        need = self.min_set * max(self.max_its - self._done, int(nIterations), 0)
        vals = np.ascontiguousarray(rng.peek(need), np.int32) if need else np.zeros(0, np.int32)
        used, nm, ni, found = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        T = np.zeros(16, np.float32)
        inl = np.zeros(max(self.n, 1), np.uint8)
        check(_lib.lib().orbx_pnp_iterate(self._h, int(nIterations), ptr(vals), len(vals), C.byref(used),
                                          C.byref(nm), ptr(T), ptr(inl), C.byref(ni), C.byref(found)),
              "orbx_pnp_iterate")
        rng.advance(used.value)
        self._done += used.value // self.min_set
        return (T.reshape(4, 4) if found.value else None), bool(nm.value), inl[:self.n].astype(bool), ni.value


def _rand_state(rng):
    st = _lib.RandState()
    w = rng.state_words()
    for k in range(34):
        st.r[k] = w[k]
    st.i = 34
    return st


def _rand_restore(rng, st):
    i = st.i
    rng.set_state_words([st.r[(i - 34 + k) % 34] for k in range(34)])


def _pnp_outputs(solvers, res, inl):
    out = []
    for s, r, b in zip(solvers, res, inl):
        s._done += r.used // s.min_set
        T = np.ctypeslib.as_array(r.Tcw).reshape(4, 4).copy() if r.found else None
        out.append((T, bool(r.no_more), b[:s.n].astype(bool), int(r.n_inliers)))
    return out


def pnp_iterate_candidates(solvers, nIterations, rng, raw_results=None):
    """Tracking::Relocalization's candidate loop (src/Tracking.cc:1738-1757) in one call:
    solvers[0].iterate(n), solvers[1].iterate(n), ... on the shared stream `rng` (GlibcRand),
    stopping after the first that returns a pose.  Returns (stopped, [(Tcw|None, bNoMore,
    vbInliers, nInliers)] for solvers[0..stopped]); rng advances by exactly what was drawn.
    raw_results: optional list that receives every solver's orbx_pnp_result (tests)."""
    n = len(solvers)
    hs = (C.c_void_p * max(n, 1))(*[s._h for s in solvers])
    res = (_lib.PnpResult * max(n, 1))()
    inl = [np.zeros(max(s.n, 1), np.uint8) for s in solvers]
    ip = (C.c_void_p * max(n, 1))(*[ptr(b) for b in inl])
    st = _rand_state(rng)
    stopped = C.c_int()
    check(_lib.lib().orbx_pnp_iterate_candidates(hs, n, int(nIterations), C.byref(st), res, ip, C.byref(stopped)),
          "orbx_pnp_iterate_candidates")
    _rand_restore(rng, st)
    if raw_results is not None:
        raw_results.extend(res[i] for i in range(n))
    k = min(stopped.value + 1, n)
    return stopped.value, _pnp_outputs(solvers[:k], res[:k], inl[:k])


def sim3_iterate_candidates(solvers, nIterations, rng, raw_results=None):
    """One sweep of LoopClosing::ComputeSim3's solver loop (src/LoopClosing.cc:372-402) in one call:
    solvers[0].iterate(n), solvers[1].iterate(n), ... on the shared stream `rng` (GlibcRand), stopping
    after the first that returns a Sim3; the caller resumes with solvers[stopped+1:] after its
    SearchBySim3 / OptimizeSim3.  Returns (stopped, [(T12|None, bNoMore, vbInliers[mN1], nInliers)] for
    solvers[0..stopped]); rng advances by exactly what was drawn.  raw_results: optional list that
    receives every solver's orbx_sim3_result (tests)."""
    n = len(solvers)
    hs = (C.c_void_p * max(n, 1))(*[s._h for s in solvers])
    res = (_lib.Sim3Result * max(n, 1))()
    inl = [np.zeros(max(s.n, 1), np.uint8) for s in solvers]
    ip = (C.c_void_p * max(n, 1))(*[ptr(b) for b in inl])
    st = _rand_state(rng)
    stopped = C.c_int()
    check(_lib.lib().orbx_sim3_iterate_candidates(hs, n, int(nIterations), C.byref(st), res, ip, C.byref(stopped)),
          "orbx_sim3_iterate_candidates")
    _rand_restore(rng, st)
    if raw_results is not None:
        raw_results.extend(res[i] for i in range(n))
    k = min(stopped.value + 1, n)
    return stopped.value, [s._output(r, b) for s, r, b in zip(solvers[:k], res[:k], inl[:k])]


def sim3_iterate_many(solvers, nIterations, rngs):
    """iterate(n) on independent Sim3Solvers, rngs[i] its own GlibcRand stream; one batched call."""
    n = len(solvers)
    hs = (C.c_void_p * max(n, 1))(*[s._h for s in solvers])
    res = (_lib.Sim3Result * max(n, 1))()
    inl = [np.zeros(max(s.n, 1), np.uint8) for s in solvers]
    ip = (C.c_void_p * max(n, 1))(*[ptr(b) for b in inl])
    sts = [_rand_state(r) for r in rngs]
    sp = (C.c_void_p * max(n, 1))(*[C.addressof(x) for x in sts])
    check(_lib.lib().orbx_sim3_iterate_many(hs, n, int(nIterations), sp, res, ip), "orbx_sim3_iterate_many")
    for r, x in zip(rngs, sts):
        _rand_restore(r, x)
    return [s._output(r, b) for s, r, b in zip(solvers, res[:n], inl)]


class Sim3Solver:
    """Sim3Solver (include/Sim3Solver.h:36-50) over orbx_sim3_*.

    Correspondences are given in the constructor's gather order (src/Sim3Solver.cc:37-125): the
    camera-frame points mvX3Dc1 / mvX3Dc2, mvLevelSigma2[octave] of the two keypoints, K1 / K2 as
    (fx, fy, cx, cy), and mvnIndices1 with mN1 = len(vpMatched12) so vbInliers comes back with the
    reference's length and indexing.  Like the reference the constructor applies
    SetRansacParameters() with its defaults (0.99, 6, 300); LoopClosing sets (0.99, 20, 300)."""

    def __init__(self, x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2, bFixScale, mvnIndices1=None, mN1=None, device=0):
        self._set_problem(x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2, bFixScale, mvnIndices1, mN1, device)
        prm = _lib.Sim3Params(0.99, 6, 300)
        h = C.c_void_p()
        check(_lib.lib().orbx_sim3_create(C.byref(self._struct()), C.byref(prm), self.device, C.byref(h)),
              "orbx_sim3_create")
        self._h = h
        self._read_params()

    def _set_problem(self, x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2, bFixScale, mvnIndices1, mN1, device):
        self.x3dc1 = np.ascontiguousarray(x3dc1, np.float32).reshape(-1, 3)
        self.x3dc2 = np.ascontiguousarray(x3dc2, np.float32).reshape(-1, 3)
        self.sigma2_1 = np.ascontiguousarray(sigma2_1, np.float32).reshape(-1)
        self.sigma2_2 = np.ascontiguousarray(sigma2_2, np.float32).reshape(-1)
        self.n = len(self.x3dc1)
        if not (len(self.x3dc2) == len(self.sigma2_1) == len(self.sigma2_2) == self.n):
            raise ValueError("Sim3Solver: correspondence arrays differ in length")
        self.K1 = tuple(float(v) for v in K1)
        self.K2 = tuple(float(v) for v in K2)
        self.bFixScale = bool(bFixScale)
        self.mvnIndices1 = (np.arange(self.n) if mvnIndices1 is None else np.asarray(mvnIndices1, np.int64)).reshape(-1)
        self.mN1 = self.n if mN1 is None else int(mN1)
        self.device = int(device)
        self._h = None

    def _struct(self):
        return _lib.Sim3SolverProblem(self.n, ptr(self.x3dc1), ptr(self.x3dc2), ptr(self.sigma2_1), ptr(self.sigma2_2),
                                      *self.K1, *self.K2, int(self.bFixScale))

    def _read_params(self):
        a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(_lib.lib().orbx_sim3_get_params(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)),
              "orbx_sim3_get_params")
        self.mRansacMinInliers, self.mRansacMaxIts, self.mnIterations, self.mnBestInliers = (a.value, b.value, c.value,
                                                                                          d.value)

    @classmethod
    def create_many(cls, problems, probability=0.99, minInliers=6, maxIterations=300, device=0):
        """len(problems) solvers (dicts x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2, bFixScale and optionally
        mvnIndices1, mN1) with one parameter set, by one orbx_sim3_create_many call (one upload)."""
        n = len(problems)
        objs, structs = [], (_lib.Sim3SolverProblem * max(n, 1))()
        for i, P in enumerate(problems):
            o = cls.__new__(cls)
            o._set_problem(P["x3dc1"], P["x3dc2"], P["sigma2_1"], P["sigma2_2"], P["K1"], P["K2"], P["bFixScale"],
                           P.get("mvnIndices1"), P.get("mN1"), device)
            structs[i] = o._struct()
            objs.append(o)
        prm = _lib.Sim3Params(float(probability), int(minInliers), int(maxIterations))
        hs = (C.c_void_p * max(n, 1))()
        check(_lib.lib().orbx_sim3_create_many(structs, n, C.byref(prm), int(device), hs), "orbx_sim3_create_many")
        for o, h in zip(objs, hs):
            o._h = C.c_void_p(h)
            o._read_params()
        return objs

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().orbx_sim3_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        """src/Sim3Solver.cc:127-151; resets mnIterations to 0 as the reference does."""
        prm = _lib.Sim3Params(float(probability), int(minInliers), int(maxIterations))
        check(_lib.lib().orbx_sim3_set_ransac_parameters(self._h, C.byref(prm)), "orbx_sim3_set_ransac_parameters")
        self._read_params()

    def _output(self, r, inl):
        self._read_params()
        vb = np.zeros(self.mN1, bool)
        if r.found:
            vb[self.mvnIndices1[inl[:self.n] != 0]] = True
        T = np.ctypeslib.as_array(r.T12).reshape(4, 4).copy() if r.found else None
        return T, bool(r.no_more), vb, int(r.n_inliers)

    def iterate(self, nIterations, rng):
        """iterate(nIterations, bNoMore, vbInliers, nInliers), src/Sim3Solver.cc:153-239.  rng: a rand()
        stream (glibc_rand.GlibcRand(1) is the reference's unseeded process rand()).  Returns
        (T12[4,4] or None, bNoMore, vbInliers[mN1] bool, nInliers); the stream advances by exactly
        what was drawn."""
        st = _rand_state(rng)
        nm, ni, found = C.c_int(), C.c_int(), C.c_int()
        r = _lib.Sim3Result()
        inl = np.zeros(max(self.n, 1), np.uint8)
        check(_lib.lib().orbx_sim3_iterate_stream(self._h, int(nIterations), C.byref(st), C.byref(nm), r.T12,
                                                  ptr(inl), C.byref(ni), C.byref(found)), "orbx_sim3_iterate_stream")
        _rand_restore(rng, st)
        r.no_more, r.found, r.n_inliers = nm.value, found.value, ni.value
        return self._output(r, inl)

    def iterate_values(self, nIterations, rand_vals):
        """The same from explicit rand() values (orbx_sim3_iterate); returns (used, *iterate's tuple)."""
        vals = np.ascontiguousarray(rand_vals, np.int32)
        used, nm, ni, found = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        r = _lib.Sim3Result()
        inl = np.zeros(max(self.n, 1), np.uint8)
        check(_lib.lib().orbx_sim3_iterate(self._h, int(nIterations), ptr(vals), len(vals), C.byref(used),
                                           C.byref(nm), r.T12, ptr(inl), C.byref(ni), C.byref(found)),
              "orbx_sim3_iterate")
        r.no_more, r.found, r.n_inliers = nm.value, found.value, ni.value
        return (used.value,) + self._output(r, inl)

    def find(self, rng):
        """find(vbInliers12, nInliers), src/Sim3Solver.cc:241-245: iterate(mRansacMaxIts).  Returns
        (T12 or None, vbInliers12, nInliers)."""
        T, _, vb, ni = self.iterate(self.mRansacMaxIts, rng)
        return T, vb, ni

    def _estimate(self):
        R, t, s = np.zeros(9, np.float32), np.zeros(3, np.float32), C.c_float()
        check(_lib.lib().orbx_sim3_get_estimate(self._h, ptr(R), ptr(t), C.byref(s)), "orbx_sim3_get_estimate")
        return R.reshape(3, 3), t, s.value

    def GetEstimatedRotation(self):
        return self._estimate()[0]

    def GetEstimatedTranslation(self):
        return self._estimate()[1]

    def GetEstimatedScale(self):
        return self._estimate()[2]


class Initializer:
    """Initializer (include/Initializer.h:36-45, src/Initializer.cc) over orbx_initializer_*.

    Initializer(keys_un, K, sigma=1.0, iterations=200): keys_un is mvKeysUn of the reference frame as
    [n1, 2] (x, y), K the 3x3 calibration.  Tracking creates it as Initializer(mCurrentFrame, 1.0, 200)
    (src/Tracking.cc:683).  The object is reused for every later frame, as the reference's is."""

    def __init__(self, keys_un, K, sigma=1.0, iterations=200, device=0):
        self.mvKeys1 = np.ascontiguousarray(keys_un, np.float32).reshape(-1, 2)
        self.mK = np.ascontiguousarray(K, np.float32).reshape(3, 3)
        self.mSigma = float(sigma)
        self.mMaxIterations = int(iterations)
        self.device = int(device)
        self.result = None
        h = C.c_void_p()
        check(_lib.lib().orbx_initializer_create(ptr(self.mvKeys1), len(self.mvKeys1), ptr(self.mK), self.mSigma,
                                                 self.mMaxIterations, self.device, C.byref(h)),
              "orbx_initializer_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().orbx_initializer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _buffers(self, keys_un2, vMatches12):
        k2 = np.ascontiguousarray(keys_un2, np.float32).reshape(-1, 2)
        vm = np.ascontiguousarray(vMatches12, np.int32).reshape(-1)
        if len(vm) != len(self.mvKeys1):
            raise ValueError("Initializer: vMatches12 must have one entry per reference keypoint")
        n1, N = len(self.mvKeys1), int((vm >= 0).sum())
        res = _lib.InitializerResult()
        mh, mf = np.zeros(max(N, 1), np.uint8), np.zeros(max(N, 1), np.uint8)
        res.inliers_h, res.inliers_f = ptr(mh), ptr(mf)
        out = (np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros(3 * n1, np.float32), np.zeros(n1, np.uint8))
        return k2, vm, res, mh, mf, out

    def _output(self, res, mh, mf, out):
        N = res.n_matches
        self.result = {"ok": bool(res.ok), "degenerate": bool(res.degenerate), "SH": np.float32(res.SH),
                       "SF": np.float32(res.SF), "H21": np.array(res.H21, np.float32).reshape(3, 3),
                       "F21": np.array(res.F21, np.float32).reshape(3, 3), "itH": res.it_h, "itF": res.it_f,
                       "model": res.model, "n_hyp": res.n_hyp, "nGood": np.array(res.n_good, np.int32),
                       "parallax": np.array(res.parallax, np.float32), "best": res.best, "N": N,
                       "n_inliers": res.n_inliers, "maskH": mh[:N].astype(bool), "maskF": mf[:N].astype(bool)}
        if not res.ok:
            return False, None, None, None, None
        R, t, p, tri = out
        return True, R.reshape(3, 3), t, p.reshape(-1, 3), tri.astype(bool)

    def Initialize(self, keys_un2, vMatches12, rng):
        """Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated), src/Initializer.cc:58-167.
        keys_un2: mvKeysUn of the current frame [n2, 2]; vMatches12[n1]: index into it or -1; rng: the
        process rand() stream (the reference seeds it with DUtils::Random::SeedRandOnce(0): GlibcRand(0)),
        advanced by the 8 * iterations values drawn.  Returns (ok, R21 [3,3], t21 [3], vP3D [n1,3],
        vbTriangulated [n1]); the last four are None when ok is False.  Fewer than 8 matches raise
        OrbxError (the reference underflows there).  self.result keeps the stage results."""
        k2, vm, res, mh, mf, out = self._buffers(keys_un2, vMatches12)
        st = _rand_state(rng)
        check(_lib.lib().orbx_initializer_initialize_stream(self._h, ptr(k2), len(k2), ptr(vm), C.byref(st),
                                                            ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]),
                                                            C.byref(res)), "orbx_initializer_initialize_stream")
        _rand_restore(rng, st)
        return self._output(res, mh, mf, out)

    def initialize_values(self, keys_un2, vMatches12, rand_vals, sentinel=None):
        """The same from explicit rand() values (orbx_initializer_initialize); returns (used, raw output
        buffers (R21, t21, p3d, triangulated), *Initialize's tuple).  sentinel: a byte the raw buffers are
        pre-filled with, to see what a false return leaves untouched."""
        k2, vm, res, mh, mf, out = self._buffers(keys_un2, vMatches12)
        if sentinel is not None:
            for b in out:
                b.view(np.uint8)[:] = sentinel
        vals = np.ascontiguousarray(rand_vals, np.int32)
        used = C.c_int()
        check(_lib.lib().orbx_initializer_initialize(self._h, ptr(k2), len(k2), ptr(vm), ptr(vals), len(vals),
                                                     C.byref(used), ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                                     ptr(out[3]), C.byref(res)), "orbx_initializer_initialize")
        return (used.value, out) + self._output(res, mh, mf, out)


def pnp_iterate_many(solvers, nIterations, rngs):
    """iterate(n) on independent solvers, rngs[i] its own GlibcRand stream; one batched call."""
    n = len(solvers)
    hs = (C.c_void_p * max(n, 1))(*[s._h for s in solvers])
    res = (_lib.PnpResult * max(n, 1))()
    inl = [np.zeros(max(s.n, 1), np.uint8) for s in solvers]
    ip = (C.c_void_p * max(n, 1))(*[ptr(b) for b in inl])
    sts = [_rand_state(r) for r in rngs]
    sp = (C.c_void_p * max(n, 1))(*[C.addressof(x) for x in sts])
    check(_lib.lib().orbx_pnp_iterate_many(hs, n, int(nIterations), sp, res, ip), "orbx_pnp_iterate_many")
    for r, x in zip(rngs, sts):
        _rand_restore(r, x)
    return _pnp_outputs(solvers, res[:n], inl)


class ORBVocabulary:
    """DBoW2 TemplatedVocabulary<FORB> (include/ORBVocabulary.h) on the GPU:
    loadFromTextFile (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1420) and
    transform(features, BowVector, FeatureVector, levelsup) (:1125-1196) over liborbx.so."""

    def __init__(self, device=0):
        self.device = device
        self._h = None
        self._score_db = None
        self._score_lock = threading.Lock()

    def loadFromText(self, text):
        """The text of a vocabulary file (ORBvoc.txt format).  Returns True like the reference."""
        self.close()
        raw = text.encode() if isinstance(text, str) else bytes(text)
        h = C.c_void_p()
        check(_lib.lib().orbx_voc_load_text(raw, len(raw), self.device, C.byref(h)), "orbx_voc_load_text")
        self._h = h
        info = np.zeros(6, np.int32)
        check(_lib.lib().orbx_voc_info(h, ptr(info)), "orbx_voc_info")
        self.k, self.L, self.scoring, self.weighting, self.n_nodes, self.n_words = (int(x) for x in info)
        return True

    def loadFromTextFile(self, path):
        with open(path, "rb") as f:
            return self.loadFromText(f.read())

    def transform_sets(self, desc_sets, levelsup=4):
        """Batch form: list of (n_i, 32) uint8 descriptor arrays -> list of
        (bow_words, bow_values, fv_nodes, fv_off, fv_feat) per set (std::map order)."""
        sets = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in desc_sets]
        off = np.zeros(len(sets) + 1, np.int32)
        off[1:] = np.cumsum([len(d) for d in sets])
        total = int(off[-1])
        desc = np.concatenate(sets) if total else np.zeros((1, 32), np.uint8)
        m = max(total, 1)
        bw, bv = np.zeros(m, np.uint32), np.zeros(m, np.float64)
        fn, fo, ff = np.zeros(m, np.uint32), np.zeros(m + len(sets), np.int32), np.zeros(m, np.int32)
        nb, nf = np.zeros(len(sets), np.int32), np.zeros(len(sets), np.int32)
        check(_lib.lib().orbx_voc_transform(self._h, ptr(desc), ptr(off), len(sets), int(levelsup), ptr(bw), ptr(bv),
                                            ptr(nb), ptr(fn), ptr(fo), ptr(ff), ptr(nf)), "orbx_voc_transform")
        out = []
        for s in range(len(sets)):
            o, b, q = int(off[s]), int(nb[s]), int(nf[s])
            foff = fo[o + s:o + s + q + 1].copy()
            out.append((bw[o:o + b].copy(), bv[o:o + b].copy(), fn[o:o + q].copy(), foff,
                        ff[o:o + int(foff[-1] if q else 0)].copy()))
        return out

    def transform(self, desc, levelsup=4):
        """(BowVector as (words, values), FeatureVector as CSR (nodes, off, feat))."""
        return self.transform_sets([desc], levelsup)[0]

    def score(self, v1_words, v1_values, v2_words, v2_values):
        """ORBVocabulary::score(v1, v2) (DBoW2 L1Scoring::score) of two BowVectors given as ascending
        word ids and values: the reference's double, computed on the GPU (v2 goes through a private
        one-keyframe KeyFrameDatabase; KeyFrameDatabase.score scores many keyframes at once).  Calls are
        serialised by a lock; each costs two small uploads, three launches and a read-back."""
        with self._score_lock:
            if self._score_db is None:
                self._score_db = KeyFrameDatabase(self)
                self._score_db.voc = None  # no reference cycle: the vocabulary owns this database
            db = self._score_db
            db.add(0, (v2_words, v2_values))
            try:
                return float(db.score((v1_words, v1_values), [0])[0])
            finally:
                db.erase(0)

    def close(self):
        if getattr(self, "_score_db", None) is not None:
            self._score_db.close()
            self._score_db = None
        if getattr(self, "_h", None):
            _lib.lib().orbx_voc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _bow(bow):
    w = np.ascontiguousarray(bow[0], np.uint32).reshape(-1)
    v = np.ascontiguousarray(bow[1], np.float64).reshape(-1)
    if len(w) != len(v):
        raise ValueError("BowVector words and values differ in length")
    return w, v


class KeyFrameDatabase:
    """The reference's KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:33-341) on
    the GPU over orbx_kfdb_*: the same candidate lists in the same order, and the six KeyFrame members
    the queries touch (mnRelocQuery, mnRelocWords, mRelocScore, mnLoopQuery, mnLoopWords, mLoopScore)
    kept on the device per keyframe id (read_state).  A keyframe is its mnId; a BowVector is a pair
    (ascending word ids, values) as ORBVocabulary.transform returns it.  Raises OrbxError (code -4)
    without a GPU -- there is no CPU fallback."""

    def __init__(self, voc, device=None):
        h = C.c_void_p()
        dev = int(voc.device if device is None else device)
        check(_lib.lib().orbx_kfdb_create(getattr(voc, "_h", None), dev, C.byref(h)), "orbx_kfdb_create")
        self._h = h
        self.voc = voc

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().orbx_kfdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, kf_id, bow):
        """add(pKF): kf_id = pKF->mnId, bow = pKF->mBowVec."""
        w, v = _bow(bow)
        check(_lib.lib().orbx_kfdb_add(self._h, int(kf_id), ptr(w), ptr(v), len(w)), "orbx_kfdb_add")

    def erase(self, kf_id):
        check(_lib.lib().orbx_kfdb_erase(self._h, int(kf_id)), "orbx_kfdb_erase")

    def clear(self):
        check(_lib.lib().orbx_kfdb_clear(self._h), "orbx_kfdb_clear")

    def set_neighbours(self, neighbours):
        """neighbours: {kf_id: GetBestCovisibilityKeyFrames(10) as ids, in the graph's order}."""
        ids = np.array(list(neighbours.keys()), np.int64)
        best = np.zeros((max(len(ids), 1), 10), np.int64)
        nb = np.zeros(max(len(ids), 1), np.int32)
        for i, k in enumerate(ids):
            lst = [int(x) for x in neighbours[int(k)]]
            if len(lst) > 10:
                raise ValueError("more than 10 neighbours")
            best[i, :len(lst)] = lst
            nb[i] = len(lst)
        check(_lib.lib().orbx_kfdb_set_neighbours(self._h, ptr(ids), ptr(best), ptr(nb), len(ids)),
              "orbx_kfdb_set_neighbours")

    def size(self):
        """(live keyframes, pool entries in use)."""
        live, pool = C.c_int(), C.c_longlong()
        check(_lib.lib().orbx_kfdb_size(self._h, C.byref(live), C.byref(pool)), "orbx_kfdb_size")
        return live.value, pool.value

    def _cap(self, cap):
        return max(self.size()[0], 1) if cap is None else int(cap)

    def DetectRelocalizationCandidates(self, frame_id, bow, cap=None):
        """DetectRelocalizationCandidates(F): frame_id = F->mnId, bow = F->mBowVec -> keyframe ids."""
        w, v = _bow(bow)
        cap = self._cap(cap)
        cand, n = np.zeros(max(cap, 1), np.int64), C.c_int()
        check(_lib.lib().orbx_kfdb_reloc_candidates(self._h, int(frame_id), ptr(w), ptr(v), len(w), ptr(cand), cap,
                                                    C.byref(n)), "orbx_kfdb_reloc_candidates")
        return [int(x) for x in cand[:n.value]]

    def DetectLoopCandidates(self, kf_mnid, bow, connected, minScore, cap=None):
        """DetectLoopCandidates(pKF, minScore): connected = pKF->GetConnectedKeyFrames() as ids."""
        w, v = _bow(bow)
        conn = np.ascontiguousarray(list(connected), np.int64)
        cap = self._cap(cap)
        cand, n = np.zeros(max(cap, 1), np.int64), C.c_int()
        check(_lib.lib().orbx_kfdb_loop_candidates(self._h, int(kf_mnid), ptr(w), ptr(v), len(w), ptr(conn), len(conn),
                                                   float(minScore), ptr(cand), cap, C.byref(n)),
              "orbx_kfdb_loop_candidates")
        return [int(x) for x in cand[:n.value]]

    def score(self, bow, kf_ids):
        """mpVoc->score(bow, pKF->mBowVec) for each listed (live) keyframe: float64 array."""
        w, v = _bow(bow)
        ids = np.ascontiguousarray(list(kf_ids), np.int64)
        out = np.zeros(max(len(ids), 1), np.float64)
        check(_lib.lib().orbx_kfdb_score(self._h, ptr(w), ptr(v), len(w), ptr(ids), len(ids), ptr(out)),
              "orbx_kfdb_score")
        return out[:len(ids)]

    def read_state(self, kf_ids):
        """The six members of the listed keyframes: dict of arrays named like the reference's members."""
        ids = np.ascontiguousarray(list(kf_ids), np.int64)
        m = max(len(ids), 1)
        out = dict(mnRelocQuery=np.zeros(m, np.uint64), mnRelocWords=np.zeros(m, np.int32),
                   mRelocScore=np.zeros(m, np.float32), mnLoopQuery=np.zeros(m, np.uint64),
                   mnLoopWords=np.zeros(m, np.int32), mLoopScore=np.zeros(m, np.float32))
        check(_lib.lib().orbx_kfdb_read_state(self._h, ptr(ids), len(ids), *[ptr(a) for a in out.values()]),
              "orbx_kfdb_read_state")
        return {k: a[:len(ids)] for k, a in out.items()}

    def reloc_candidates_device(self, frame_id, words, values, n, cand, n_cand, stream=None):
        """DetectRelocalizationCandidates queued on `stream` (a torch stream; None: the handle's own)
        with no host synchronisation: words (uint32 as int32) / values (float64) / n (int32) are device
        tensors laid out as orbx_voc_transform_device writes one set, cand (int64) and n_cand (int32)
        device tensors that receive the ids and their number."""
        check(_lib.lib().orbx_kfdb_reloc_candidates_device(self._h, int(frame_id), ptr(words), ptr(values), ptr(n),
                                                           ptr(cand), int(cand.numel()), ptr(n_cand),
                                                           _stream_ptr(stream, True)),
              "orbx_kfdb_reloc_candidates_device")

    def loop_candidates_device(self, kf_mnid, words, values, n, connected, minScore, cand, n_cand, stream=None):
        """DetectLoopCandidates queued on `stream`; connected is a host list of ids."""
        conn = np.ascontiguousarray(list(connected), np.int64)
        check(_lib.lib().orbx_kfdb_loop_candidates_device(self._h, int(kf_mnid), ptr(words), ptr(values), ptr(n),
                                                          ptr(conn), len(conn), float(minScore), ptr(cand),
                                                          int(cand.numel()), ptr(n_cand), _stream_ptr(stream, True)),
              "orbx_kfdb_loop_candidates_device")


class CovisibilityMap:
    """The covisibility relation on the GPU over orbx_covis_*: a device-resident observation table (one row
    per keyframe: MapPoint ids, octaves, the stereo and close flags; nObs and bad per point) and the four
    queries that read it -- KeyFrame::UpdateConnections steps 1-2 (src/KeyFrame.cc:367-467), the vote of
    Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1523-1581), Tracking::UpdateLocalPoints (:1483-1515)
    and LocalMapping::KeyFrameCulling (src/LocalMapping.cc:784-871) -- with the reference's exact counts,
    orders and verdicts.  Keyframes and points are their mnIds.  Raises OrbxError (code -4) without a GPU --
    there is no CPU fallback."""

    STEREO, CLOSE = 1, 2
    KEPT, CULLED, TO_BE_ERASED = 0, 1, 2

    def __init__(self, device=0):
        h = C.c_void_p()
        check(_lib.lib().orbx_covis_create(int(device), C.byref(h)), "orbx_covis_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().orbx_covis_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        check(_lib.lib().orbx_covis_clear(self._h), "orbx_covis_clear")

    @staticmethod
    def flags(u_right, depth, th_depth):
        """The two flag bits from mvuRight / mvDepth / mThDepth, as the reference tests them."""
        u, d = np.asarray(u_right, np.float32), np.asarray(depth, np.float32)
        return ((u >= 0).astype(np.uint8) * CovisibilityMap.STEREO |
                (~((d > np.float32(th_depth)) | (d < 0))).astype(np.uint8) * CovisibilityMap.CLOSE)

    def set_keyframe(self, kf_id, point_ids, octaves, flags):
        """Inserts or replaces the keyframe's whole row (point id -1: no MapPoint)."""
        p = np.ascontiguousarray(point_ids, np.int32).reshape(-1)
        o = np.ascontiguousarray(octaves, np.int32).reshape(-1)
        f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        if not (len(p) == len(o) == len(f)):
            raise ValueError("row arrays differ in length")
        check(_lib.lib().orbx_covis_set_keyframe(self._h, int(kf_id), len(p), ptr(p), ptr(o), ptr(f)),
              "orbx_covis_set_keyframe")

    def erase_keyframe(self, kf_id):
        check(_lib.lib().orbx_covis_erase_keyframe(self._h, int(kf_id)), "orbx_covis_erase_keyframe")

    def set_points_bad(self, ids):
        a = np.ascontiguousarray(list(ids), np.int32)
        check(_lib.lib().orbx_covis_set_points_bad(self._h, ptr(a), len(a)), "orbx_covis_set_points_bad")

    def size(self):
        """(live keyframes, pool entries in use, largest point id + 1)."""
        live, pool, npts = C.c_int(), C.c_longlong(), C.c_int()
        check(_lib.lib().orbx_covis_size(self._h, C.byref(live), C.byref(pool), C.byref(npts)), "orbx_covis_size")
        return live.value, pool.value, npts.value

    def read_keyframe(self, kf_id):
        """The row as set, a bad point shown as -1: (point_ids, octaves, flags)."""
        n, L = C.c_int(), _lib.lib()
        rc = L.orbx_covis_read_keyframe(self._h, int(kf_id), None, None, None, 0, C.byref(n))
        if rc not in (_lib.ORBX_OK, _lib.ORBX_ERR_CAPACITY):
            check(rc, "orbx_covis_read_keyframe")
        m = max(n.value, 1)
        p, o, f = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.uint8)
        check(L.orbx_covis_read_keyframe(self._h, int(kf_id), ptr(p), ptr(o), ptr(f), m, C.byref(n)),
              "orbx_covis_read_keyframe")
        return p[:n.value], o[:n.value], f[:n.value]

    def read_points(self, ids):
        """(nObs, bad) of the listed points."""
        a = np.ascontiguousarray(list(ids), np.int32)
        nobs, bad = np.zeros(max(len(a), 1), np.int32), np.zeros(max(len(a), 1), np.uint8)
        check(_lib.lib().orbx_covis_read_points(self._h, ptr(a), len(a), ptr(nobs), ptr(bad)),
              "orbx_covis_read_points")
        return nobs[:len(a)], bad[:len(a)]

    def update_connections(self, kf_id, th=15):
        """UpdateConnections steps 1-2: (KFcounter as [(kf, count)] ids ascending, the ordered list as
        [(kf, weight)] weight descending / id descending, or the single (pKFmax, nmax) when none reaches th)."""
        cap = max(self.size()[0], 1)
        ck, cw = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
        ok, ow = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
        nc, no = C.c_int(), C.c_int()
        check(_lib.lib().orbx_covis_update_connections(self._h, int(kf_id), int(th), ptr(ck), ptr(cw), cap,
                                                       C.byref(nc), ptr(ok), ptr(ow), cap, C.byref(no)),
              "orbx_covis_update_connections")
        return (list(zip(ck[:nc.value].tolist(), cw[:nc.value].tolist())),
                list(zip(ok[:no.value].tolist(), ow[:no.value].tolist())))

    def vote(self, point_ids):
        """The vote of UpdateLocalKeyFrames: (was_bad bytes, keyframeCounter as [(kf, count)] ids ascending,
        pKFmax or None, max)."""
        p = np.ascontiguousarray(point_ids, np.int32).reshape(-1)
        cap = max(self.size()[0], 1)
        wb = np.zeros(max(len(p), 1), np.uint8)
        k, c = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
        n, kmax, nmax = C.c_int(), C.c_int64(), C.c_int32()
        check(_lib.lib().orbx_covis_vote(self._h, ptr(p), len(p), ptr(wb), ptr(k), ptr(c), cap, C.byref(n),
                                         C.byref(kmax), C.byref(nmax)), "orbx_covis_vote")
        return (wb[:len(p)], list(zip(k[:n.value].tolist(), c[:n.value].tolist())),
                None if kmax.value < 0 else kmax.value, nmax.value)

    def local_points(self, kf_ids, cap=None):
        """UpdateLocalPoints: the distinct non-bad points of the listed keyframes, first occurrence first."""
        ids = np.ascontiguousarray(list(kf_ids), np.int64)
        cap = max(self.size()[1], 1) if cap is None else int(cap)
        out, n = np.zeros(max(cap, 1), np.int32), C.c_int()
        check(_lib.lib().orbx_covis_local_points(self._h, ptr(ids), len(ids), ptr(out), cap, C.byref(n)),
              "orbx_covis_local_points")
        return out[:n.value].tolist()

    def cull(self, cand_ids, not_erase, monocular):
        """KeyFrameCulling over the candidates in order: (verdict per candidate, points that went bad)."""
        ids = np.ascontiguousarray(list(cand_ids), np.int64)
        ne = np.ascontiguousarray([1 if x else 0 for x in not_erase], np.uint8)
        if len(ne) != len(ids):
            raise ValueError("not_erase and cand_ids differ in length")
        cap = max(self.size()[1], 1)
        v, bad, n = np.zeros(max(len(ids), 1), np.uint8), np.zeros(cap, np.int32), C.c_int()
        check(_lib.lib().orbx_covis_cull(self._h, ptr(ids), len(ids), ptr(ne), 1 if monocular else 0, ptr(v),
                                         ptr(bad), cap, C.byref(n)), "orbx_covis_cull")
        return v[:len(ids)].tolist(), bad[:n.value].tolist()


def new_points_problem(prob):
    """orbx_new_points_problem from a dict(current, neighbours, monocular, scale_factor); every keyframe
    is a dict(keys_un, desc, u_right, has_mp, node_id, node_off, feat, keys_xy, depth, mp_pos, Tcw, fx, fy,
    cx, cy, mb, mbf, scale_factors, level_sigma2) of host numpy arrays (synth.new_points_problem's
    layout) or device tensors.  Returns (problem, keep-alive)."""
    keep = []

    def arr(x, dt):
        if x is None or not isinstance(x, np.ndarray):
            return x
        a = np.ascontiguousarray(x, dt)
        keep.append(a)
        return a

    def kf(d, k):
        t = k.kf
        t.n = len(d["desc"])
        t.keys_un, t.desc = ptr(arr(d["keys_un"], KEYPOINT_DTYPE)), ptr(arr(d["desc"], np.uint8))
        t.u_right, t.has_mp = ptr(arr(d.get("u_right"), np.float32)), ptr(arr(d.get("has_mp"), np.uint8))
        t.n_nodes = len(d["node_id"])
        t.node_id, t.node_off = ptr(arr(d["node_id"], np.uint32)), ptr(arr(d["node_off"], np.int32))
        t.feat = ptr(arr(d["feat"], np.int32))
        k.keys_xy, k.depth = ptr(arr(d.get("keys_xy"), np.float32)), ptr(arr(d.get("depth"), np.float32))
        k.mp_pos = ptr(arr(d.get("mp_pos"), np.float32))
        k.Tcw[:] = _f32(d["Tcw"]).reshape(16).tolist()
        for f in ("fx", "fy", "cx", "cy", "mb", "mbf"):
            setattr(k, f, float(d[f]))
        nl = len(d["scale_factors"])
        k.n_levels = nl
        sf, sg = np.zeros(16, np.float32), np.zeros(16, np.float32)
        sf[:nl], sg[:nl] = d["scale_factors"], d["level_sigma2"]
        k.scale_factors[:] = sf.tolist()
        k.level_sigma2[:] = sg.tolist()

    p = _lib.NewPointsProblem()
    kf(prob["current"], p.current)
    nn = len(prob["neighbours"])
    nbs = (_lib.NewPointsKF * max(1, nn))()
    for i, d in enumerate(prob["neighbours"]):
        kf(d, nbs[i])
    keep.append(nbs)
    p.n_neighbours, p.neighbours = nn, C.cast(nbs, C.POINTER(_lib.NewPointsKF))
    p.monocular, p.scale_factor = int(bool(prob["monocular"])), float(prob["scale_factor"])
    return p, keep


NEW_POINTS_PROBES = {"exit": (0, np.uint8, ()), "cos": (1, np.float32, (3,)), "F12": (2, np.float32, None),
                     "match12": (3, np.int32, ())}


class LocalMapping:
    """LocalMapping(pMap, bMonocular)'s CreateNewMapPoints (src/LocalMapping.cc:281-558) on an explicit
    problem: the current keyframe and its GetBestCovisibilityKeyFrames(nn) neighbours, gathered as the
    reference reads them.  One call: one copy in, the chain of neighbours on the device, one copy back.
    The caller then makes the MapPoints in the returned order (:539-553)."""

    def __init__(self, monocular, device=0):
        self.mbMonocular = bool(monocular)
        self.device = device
        self._h = C.c_void_p()
        check(_lib.lib().orbx_new_points_create(device, C.byref(self._h)), "orbx_new_points_create")
        f = C.POINTER(C.c_int)()
        check(_lib.lib().orbx_new_points_stop_flag(self._h, C.byref(f)), "orbx_new_points_stop_flag")
        self._flag = f

    def close(self):
        if self._h:
            _lib.lib().orbx_new_points_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def InsertKeyFrame(self, raised=True):
        """What CheckNewKeyFrames() (:320) reads: a queued keyframe raises the handle's flag."""
        self._flag[0] = 1 if raised else 0

    def CheckNewKeyFrames(self):
        return self._flag[0] != 0

    def debug_options(self, raise_after_neighbour=-1, probes=False):
        o = _lib.NewPointsDebugOptions(int(raise_after_neighbour), int(bool(probes)))
        check(_lib.lib().orbx_debug_new_points_options(self._h, C.byref(o)), "orbx_debug_new_points_options")

    @staticmethod
    def _outputs(n1, nn):
        return dict(n_new=np.zeros(1, np.int32), neighbours_done=np.zeros(1, np.int32),
                    point_idx=np.zeros((max(1, n1), 3), np.int32), point_pos=np.zeros((max(1, n1), 3), np.float32),
                    point_normal=np.zeros((max(1, n1), 3), np.float32),
                    point_dist=np.zeros((max(1, n1), 2), np.float32), nb_skip=np.zeros(max(1, nn), np.int32),
                    nb_nmatches=np.zeros(max(1, nn), np.int32), nb_baseline=np.zeros(max(1, nn), np.float32),
                    nb_median_depth=np.zeros(max(1, nn), np.float32), has_mp1=np.zeros(max(1, n1), np.uint8))

    @staticmethod
    def _result(out, n1, nn):
        n = int(out["n_new"][0])
        return dict(n_new=n, neighbours_done=int(out["neighbours_done"][0]), points=out["point_idx"][:n].copy(),
                    pos=out["point_pos"][:n].copy(), normal=out["point_normal"][:n].copy(),
                    dist=out["point_dist"][:n].copy(), nb_skip=out["nb_skip"][:nn].copy(),
                    nb_nmatches=out["nb_nmatches"][:nn].copy(), nb_baseline=out["nb_baseline"][:nn].copy(),
                    nb_median=out["nb_median_depth"][:nn].copy(), has_mp1=out["has_mp1"][:n1].copy())

    def CreateNewMapPoints(self, problem, stop=False, use_bool=False):
        """problem: synth.new_points_problem's dict.  stop: raise the flag before the call (the first
        neighbour still runs, :320).  use_bool: go through the bool* entry point.  Returns dict(n_new,
        neighbours_done, points [n, 3] (neighbour, idx1, idx2), pos, normal, dist [n, 2] (min, max),
        nb_skip, nb_nmatches, nb_baseline, nb_median, has_mp1)."""
        prob = dict(problem, monocular=self.mbMonocular)
        p, keep = new_points_problem(prob)
        n1, nn = p.current.kf.n, p.n_neighbours
        out = self._outputs(n1, nn)
        r = _lib.NewPointsResult()
        for k in out:
            setattr(r, k, ptr(out[k]))
        L = _lib.lib()
        if use_bool:
            b = C.c_bool(bool(stop))
            check(L.orbx_create_new_map_points_bool(self._h, C.byref(p), C.byref(r), C.addressof(b)),
                  "orbx_create_new_map_points_bool")
        else:
            old = self._flag[0]
            if stop:
                self._flag[0] = 1
            try:
                check(L.orbx_create_new_map_points(self._h, C.byref(p), C.byref(r)), "orbx_create_new_map_points")
            finally:
                self._flag[0] = old
        return self._result(out, n1, nn)

    def probes(self, n1, nn):
        """The probes of the last host call (debug_options(probes=True)): exit [nn, n1], cos [nn, n1, 3],
        F12 [nn, 3, 3], match12 [nn, n1]."""
        out = {}
        for k, (what, dt, _) in NEW_POINTS_PROBES.items():
            shape = (nn, 3, 3) if k == "F12" else ((nn, n1, 3) if k == "cos" else (nn, n1))
            a = np.zeros(shape, dt)
            got = _lib.lib().orbx_debug_new_points_probe(self._h, what, ptr(a) if a.size else None, a.nbytes)
            if got != a.nbytes:
                raise _lib.OrbxError(int(got) if got < 0 else _lib.ORBX_OK, "orbx_debug_new_points_probe")
            out[k] = a
        return out


def new_points_host(problem, neighbour, match12=None):
    """orbx_debug_new_points_host: neighbour `neighbour`'s gate and, with a match12, its pairs, by the
    kernels' routines compiled for the host (no device)."""
    p, keep = new_points_problem(problem)
    n1 = p.current.kf.n
    skip, base, med = np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros(1, np.float32)
    F12 = np.zeros((3, 3), np.float32)
    ex, cos = np.zeros(max(1, n1), np.uint8), np.zeros((max(1, n1), 3), np.float32)
    pos, nrm = np.zeros((max(1, n1), 3), np.float32), np.zeros((max(1, n1), 3), np.float32)
    dist = np.zeros((max(1, n1), 2), np.float32)
    m = None if match12 is None else np.ascontiguousarray(match12, np.int32)
    check(_lib.lib().orbx_debug_new_points_host(C.byref(p), int(neighbour), ptr(m), ptr(skip), ptr(base), ptr(med),
                                                ptr(F12), ptr(ex), ptr(cos), ptr(pos), ptr(nrm), ptr(dist)),
          "orbx_debug_new_points_host")
    return dict(skip=int(skip[0]), baseline=base[0], median=med[0], F12=F12, exit=ex[:n1], cos=cos[:n1], pos=pos[:n1],
                normal=nrm[:n1], dist=dist[:n1])
