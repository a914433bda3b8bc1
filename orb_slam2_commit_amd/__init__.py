"""orb_slam2_commit_amd -- MI355X-native (gfx950 HIP) ORB-SLAM2 hot path.

The product is liborbx.so (HIP kernels + C ABI, include/orbx.h); this package
is the thin host-side mirror of the reference classes over it.
"""
from ._lib import KEYPOINT_DTYPE, OrbxError  # noqa: F401
from .orb import CovisibilityMap, Initializer, KeyFrameDatabase, LocalMapping, ORBextractor, ORBmatcher, ORBVocabulary, Optimizer, PnPsolver, Sim3Solver, compute_stereo_matches, cvt_gray, frame_rgbd, frame_stereo, rgbd_frames_device  # noqa: F401

__all__ = ["CovisibilityMap", "Initializer", "KeyFrameDatabase", "LocalMapping", "ORBextractor", "ORBmatcher", "ORBVocabulary", "Optimizer", "PnPsolver", "Sim3Solver", "compute_stereo_matches", "cvt_gray", "frame_rgbd", "frame_stereo", "rgbd_frames_device", "KEYPOINT_DTYPE", "OrbxError"]
