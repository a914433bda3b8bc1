// shim.cc -- the reference's hot-path classes (ORBextractor, Frame's ORB/stereo part, its RGB-D and
// monocular constructors, ComputeBoW, cv::cvtColor's four grey codes,
// ORBmatcher's SearchByBoW x2 / SearchByProjection x3 / SearchForTriangulation / Fuse /
// DescriptorDistance, PnPsolver, Optimizer::PoseOptimization / LocalBundleAdjustment /
// GlobalBundleAdjustemnt,
// MapPoint::ComputeDistinctiveDescriptors, ORBVocabulary) as thin C++ over the C ABI of liborbx.so
// (include/orbx.h).  Argument meaning and error behaviour follow the
// reference; a library error (no device, bad geometry) throws std::runtime_error where the
// reference would assert or crash.  No computation happens here beyond marshalling: gathering the
// inputs from the object graph and applying the results to it, as the reference's own members do.
#include <cstddef>
#include <cstdio>
#include <exception>
#include <cstring>
#include <list>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>

#include <algorithm>
#include <cmath>
#include <fstream>
#include <iterator>
#include <set>
#include <sstream>

#include "KeyFrameDatabase.h"
#include "ORBVocabulary.h"
#include "ORBextractor.h"
#include "ORBmatcher.h"
#include "Objects.h"
#include "Optimizer.h"
#include "PnPsolver.h"
#include "Initializer.h"
#include "LocalMapping.h"
#include "Sim3Solver.h"
#include "orbx.h"
#include "orbx_shim.h"

static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint layout");
static_assert(offsetof(cv::KeyPoint, octave) == offsetof(orbx_keypoint, octave), "cv::KeyPoint layout");
static_assert(offsetof(cv::KeyPoint, response) == offsetof(orbx_keypoint, response), "cv::KeyPoint layout");

namespace ORB_SLAM2 {

static void check(orbx_status s, const char* what) {
  if (s != ORBX_OK) throw std::runtime_error(std::string(what) + " failed: orbx_status " + std::to_string(s));
}

// rows of 32 bytes back to back (cv::Mat descriptors are continuous unless they are views)
static cv::Mat continuous(const cv::Mat& m) { return m.isContinuous() ? m : m.clone(); }

// ------------------------------------------------------------------ ORBextractor
ORBextractor::ORBextractor(int nfeatures_, float scaleFactor_, int nlevels_, int iniThFAST_, int minThFAST_)
    : nfeatures(nfeatures_), scaleFactor(scaleFactor_), nlevels(nlevels_), iniThFAST(iniThFAST_),
      minThFAST(minThFAST_) {
  orbx_extractor_params p{nfeatures, scaleFactor_, nlevels, iniThFAST, minThFAST};
  check(orbx_extractor_create(&p, gOrbxDevice, &mpGpu), "orbx_extractor_create");
  mvScaleFactor.resize(nlevels);
  mvInvScaleFactor.resize(nlevels);
  mvLevelSigma2.resize(nlevels);
  mvInvLevelSigma2.resize(nlevels);
  check(orbx_extractor_scale_tables(mpGpu, mvScaleFactor.data(), mvInvScaleFactor.data(), mvLevelSigma2.data(),
                                    mvInvLevelSigma2.data()),
        "orbx_extractor_scale_tables");
  // the constructor's other tables (src/ORBextractor.cc:433-490): quotas, the IC_Angle circle, pattern
  mnFeaturesPerLevel.resize(nlevels);
  umax.resize(16);  // HALF_PATCH_SIZE + 1
  std::vector<int> pts(1024);
  check(orbx_extractor_tables(mpGpu, mnFeaturesPerLevel.data(), umax.data(), pts.data()), "orbx_extractor_tables");
  pattern.resize(512);
  for (int i = 0; i < 512; i++) pattern[i] = cv::Point(pts[2 * i], pts[2 * i + 1]);
  check(orbx_extractor_set_pyramid_readback(mpGpu, 1), "orbx_extractor_set_pyramid_readback");
  mvImagePyramid.resize(nlevels);
}

ORBextractor::~ORBextractor() {
  if (mpGpu) orbx_extractor_destroy(mpGpu);
}

void ORBextractor::operator()(cv::InputArray _image, cv::InputArray, std::vector<cv::KeyPoint>& _keypoints,
                              cv::OutputArray _descriptors) {
  Extract(_image, _keypoints, _descriptors, true);
}

void ORBextractor::ExtractForFrame(const cv::Mat& image, std::vector<cv::KeyPoint>& keypoints, cv::Mat& descriptors) {
  Extract(image, keypoints, descriptors, false);
}

void ORBextractor::Extract(cv::InputArray _image, std::vector<cv::KeyPoint>& _keypoints,
                           cv::OutputArray _descriptors, bool pyramid) {
  if (_image.empty()) return;  // src/ORBextractor.cc:1141
  cv::Mat image = _image.getMat();
  if (image.type() != CV_8UC1) throw std::invalid_argument("ORBextractor: image must be CV_8UC1");  // :1145
  const int cap = orbx_extractor_max_keypoints(mpGpu, image.cols, image.rows);
  if (cap < 0) check(cap, "orbx_extractor_max_keypoints");
  _keypoints.resize(cap);
  cv::Mat desc(cap > 0 ? cap : 1, 32, CV_8U);
  int n = 0;
  check(orbx_extractor_set_pyramid_readback(mpGpu, pyramid ? 1 : 0), "orbx_extractor_set_pyramid_readback");
  check(orbx_extract(mpGpu, image.data, image.cols, image.rows, image.step,
                     reinterpret_cast<orbx_keypoint*>(_keypoints.data()), cap, desc.data, &n),
        "orbx_extract");
  _keypoints.resize(n);
  if (n == 0) {
    _descriptors.release();  // :1173
  } else {
    _descriptors.create(n, 32, CV_8U);
    cv::Mat& out = _descriptors.getMatRef();
    for (int i = 0; i < n; i++) std::memcpy(out.ptr<uint8_t>(i), desc.ptr<uint8_t>(i), 32);
  }
  for (int l = 0; l < nlevels; l++) {
    if (!pyramid) {
      mvImagePyramid[l].release();
      continue;
    }
    // new Mats every call, as ComputePyramid assigns fresh ones (an older level a caller kept stays
    // intact); the copy comes from the pinned readback orbx_extract already waited for
    int w = 0, h = 0;
    check(orbx_pyramid_level(mpGpu, 0, l, nullptr, 0, &w, &h), "orbx_pyramid_level");
    cv::Mat m(h, w, CV_8U);
    check(orbx_pyramid_level(mpGpu, 0, l, m.data, m.step, &w, &h), "orbx_pyramid_level");
    mvImagePyramid[l] = m;
  }
}

// ------------------------------------------------------------------ Frame (stereo ORB part)
float Frame::fx = 0.f, Frame::fy = 0.f, Frame::cx = 0.f, Frame::cy = 0.f, Frame::invfx = 0.f, Frame::invfy = 0.f;

Frame::Frame(const cv::Mat& imLeft, const cv::Mat& imRight, ORBextractor* extractorLeft,
             ORBextractor* extractorRight, const cv::Mat& K, const cv::Mat& distCoef, float bf, float thDepth)
    : mpORBextractorLeft(extractorLeft), mpORBextractorRight(extractorRight), mbf(bf), mThDepth(thDepth) {
  mK = K.clone();
  mDistCoef = distCoef.clone();
  ORBextractor* eL = extractorLeft;
  ORBextractor* eR = extractorRight;
  // Tracking builds both extractors with the same parameters (src/Tracking.cc:113-126): then the two
  // ExtractORB calls and ComputeStereoMatches run as one library call on the left handle (both
  // images one batch, the matcher on the device right behind them, one copy back)
  if (gOrbxFrameStereoFused && eL && eR && eL != eR && eL->nfeatures == eR->nfeatures &&
      eL->scaleFactor == eR->scaleFactor && eL->nlevels == eR->nlevels && eL->iniThFAST == eR->iniThFAST && eL->minThFAST == eR->minThFAST &&
      !imLeft.empty() && !imRight.empty() && imLeft.type() == CV_8UC1 && imRight.type() == CV_8UC1 &&
      imLeft.rows == imRight.rows && imLeft.cols == imRight.cols && K.at<float>(0, 0) != 0.f) {
    const int cap = orbx_extractor_max_keypoints(eL->gpu(), imLeft.cols, imLeft.rows);
    if (cap < 0) check(cap, "orbx_extractor_max_keypoints");
    mvKeys.resize(cap);
    mvKeysRight.resize(cap);
    cv::Mat dL(cap > 0 ? cap : 1, 32, CV_8U), dR(cap > 0 ? cap : 1, 32, CV_8U);
    std::vector<float> uR(cap > 0 ? cap : 1), dep(cap > 0 ? cap : 1);
    int nL = 0, nR = 0;
    const float fx0 = K.at<float>(0, 0);
    check(orbx_frame_stereo(eL->gpu(), imLeft.data, imLeft.step, imRight.data, imRight.step, imLeft.cols,
                            imLeft.rows, bf, bf / fx0, reinterpret_cast<orbx_keypoint*>(mvKeys.data()), dL.data, cap,
                            &nL, reinterpret_cast<orbx_keypoint*>(mvKeysRight.data()), dR.data, cap, &nR, uR.data(),
                            dep.data()),
          "orbx_frame_stereo");
    mvKeys.resize(nL);
    mvKeysRight.resize(nR);
    // ExtractForFrame's outputs: exactly n descriptor rows (none for an empty side), no pyramid kept
    if (nL) {
      mDescriptors.create(nL, 32, CV_8U);
      std::memcpy(mDescriptors.data, dL.data, (size_t)32 * nL);
    }
    if (nR) {
      mDescriptorsRight.create(nR, 32, CV_8U);
      std::memcpy(mDescriptorsRight.data, dR.data, (size_t)32 * nR);
    }
    for (int l = 0; l < eL->nlevels; l++) {
      eL->mvImagePyramid[l].release();
      eR->mvImagePyramid[l].release();
    }
    finish_stereo_frame(&uR, &dep);
    return;
  }
  // two extraction threads, each on its own extractor handle / HIP stream (src/Frame.cc:80-84)
  std::exception_ptr errL, errR;
  std::thread threadLeft([&] {
    try { ExtractORB(0, imLeft); } catch (...) { errL = std::current_exception(); }
  });
  std::thread threadRight([&] {
    try { ExtractORB(1, imRight); } catch (...) { errR = std::current_exception(); }
  });
  threadLeft.join();
  threadRight.join();
  if (errL) std::rethrow_exception(errL);
  if (errR) std::rethrow_exception(errR);
  finish_stereo_frame(nullptr, nullptr);
}

// The rest of the stereo constructor after ExtractORB (src/Frame.cc:86-123); uR / dep: the stereo
// matches orbx_frame_stereo already computed (else ComputeStereoMatches runs here)
void Frame::finish_stereo_frame(const std::vector<float>* uR, const std::vector<float>* dep) {
  N = (int)mvKeys.size();
  // scale tables (src/Frame.cc:66-73) and the static intrinsics (:111-126)
  mnScaleLevels = mpORBextractorLeft->GetLevels();
  mfScaleFactor = mpORBextractorLeft->GetScaleFactor();
  mfLogScaleFactor = std::log(mfScaleFactor);
  mvScaleFactors = mpORBextractorLeft->GetScaleFactors();
  mvInvScaleFactors = mpORBextractorLeft->GetInverseScaleFactors();
  mvLevelSigma2 = mpORBextractorLeft->GetScaleSigmaSquares();
  mvInvLevelSigma2 = mpORBextractorLeft->GetInverseScaleSigmaSquares();
  fx = mK.at<float>(0, 0);
  fy = mK.at<float>(1, 1);
  cx = mK.at<float>(0, 2);
  cy = mK.at<float>(1, 2);
  invfx = 1.0f / fx;
  invfy = 1.0f / fy;
  if (mvKeys.empty()) return;
  mb = mbf / fx;  // :133-134
  UndistortKeyPoints();
  if (uR && dep) {  // ComputeStereoMatches' results (mvKeys, mvKeysRight, mb: the same inputs)
    mvuRight.assign(uR->begin(), uR->begin() + N);
    mvDepth.assign(dep->begin(), dep->begin() + N);
  } else {
    ComputeStereoMatches();
  }
  mvpMapPoints.assign(N, nullptr);
  mvbOutlier.assign(N, false);
}

long unsigned int Frame::nNextId = 0;
float Frame::mnMinX = 0.f, Frame::mnMaxX = 0.f, Frame::mnMinY = 0.f, Frame::mnMaxY = 0.f;
float Frame::mfGridElementWidthInv = 0.f, Frame::mfGridElementHeightInv = 0.f;
bool Frame::mbInitialComputations = true;
int gOrbxDevice = 0;
bool gOrbxFrameStereoFused = true;

Frame::Frame(const cv::Mat& imLeft, const cv::Mat& imRight, const double& timeStamp, ORBextractor* extractorLeft,
             ORBextractor* extractorRight, ORBVocabulary* voc, cv::Mat& K, cv::Mat& distCoef, const float& bf,
             const float& thDepth)
    : Frame(imLeft, imRight, extractorLeft, extractorRight, K, distCoef, bf, thDepth) {
  mnId = nNextId++;
  mTimeStamp = timeStamp;
  mpORBvocabulary = voc;
  if (mvKeys.empty()) return;  // src/Frame.cc:87-88
  // :100-120 on the first frame: image bounds and the grid's cell inverses (FRAME_GRID_COLS/ROWS)
  if (mbInitialComputations) {
    ComputeImageBounds(imLeft);
    mfGridElementWidthInv = static_cast<float>(ORBX_GRID_COLS) / (mnMaxX - mnMinX);
    mfGridElementHeightInv = static_cast<float>(ORBX_GRID_ROWS) / (mnMaxY - mnMinY);
    mbInitialComputations = false;
  }
  // AssignFeaturesToGrid (:131): the matchers build the 64x48 grid on the device per call
}

// ------------------------------------------------------------------ Frame (RGB-D and monocular)
static orbx_camera frame_camera(const cv::Mat& K, const cv::Mat& distCoef) {
  orbx_camera cam;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) cam.K[3 * r + c] = K.at<float>(r, c);
  const int nd = distCoef.empty() ? 0 : distCoef.rows * distCoef.cols;
  cam.n_dist = nd < 4 ? 4 : nd;
  for (int i = 0; i < 5; i++) cam.dist[i] = i < nd ? distCoef.ptr<float>(0)[i] : 0.f;
  return cam;
}

Frame::Frame(const cv::Mat& imGray, const cv::Mat& imDepth, const double& timeStamp, ORBextractor* extractor,
             ORBVocabulary* voc, cv::Mat& K, cv::Mat& distCoef, const float& bf, const float& thDepth)
    : mpORBextractorLeft(extractor), mbf(bf), mThDepth(thDepth) {
  mK = K.clone();
  mDistCoef = distCoef.clone();
  // imDepth.at<float>(v,u), src/Frame.cc:806: the image is CV_32F by now, and a factor of 1 passes its bits on
  if (!imGray.empty() && (imGray.type() != CV_8UC1 || imDepth.type() != CV_32F))
    throw std::invalid_argument("Frame: imGray must be CV_8UC1 and imDepth CV_32F");
  init_single_camera(imGray, &imDepth, 1.0f, true, timeStamp, voc);
}

Frame::Frame(const cv::Mat& im, const cv::Mat& imDepth, const double& timeStamp, ORBextractor* extractor,
             ORBVocabulary* voc, cv::Mat& K, cv::Mat& distCoef, const float& bf, const float& thDepth,
             const float& depthMapFactor, bool bRGB)
    : mpORBextractorLeft(extractor), mbf(bf), mThDepth(thDepth) {
  mK = K.clone();
  mDistCoef = distCoef.clone();
  init_single_camera(im, &imDepth, depthMapFactor, bRGB, timeStamp, voc);
}

Frame::Frame(const cv::Mat& imGray, const double& timeStamp, ORBextractor* extractor, ORBVocabulary* voc, cv::Mat& K,
             cv::Mat& distCoef, const float& bf, const float& thDepth)
    : mpORBextractorLeft(extractor), mbf(bf), mThDepth(thDepth) {
  mK = K.clone();
  mDistCoef = distCoef.clone();
  init_single_camera(imGray, nullptr, 1.0f, true, timeStamp, voc);
}

void Frame::init_single_camera(const cv::Mat& im, const cv::Mat* imDepth, float depthMapFactor, bool bRGB,
                               const double& timeStamp, ORBVocabulary* voc) {
  mnId = nNextId++;
  mTimeStamp = timeStamp;
  mpORBvocabulary = voc;
  // scale level info (src/Frame.cc:133-140, 193-200)
  mnScaleLevels = mpORBextractorLeft->GetLevels();
  mfScaleFactor = mpORBextractorLeft->GetScaleFactor();
  mfLogScaleFactor = std::log(mfScaleFactor);
  mvScaleFactors = mpORBextractorLeft->GetScaleFactors();
  mvInvScaleFactors = mpORBextractorLeft->GetInverseScaleFactors();
  mvLevelSigma2 = mpORBextractorLeft->GetScaleSigmaSquares();
  mvInvLevelSigma2 = mpORBextractorLeft->GetInverseScaleSigmaSquares();
  if (imDepth) {
    // ExtractORB(0, imGray), UndistortKeyPoints, ComputeStereoFromRGBD (:143-154): one library call
    if (!im.empty()) {
      if (im.depth() != CV_8U || im.channels() == 2) throw std::invalid_argument("Frame: image must be CV_8UC1 / C3 / C4");
      ORBextractor* ex = mpORBextractorLeft;
      const int cap = orbx_extractor_max_keypoints(ex->gpu(), im.cols, im.rows);
      if (cap < 0) check(cap, "orbx_extractor_max_keypoints");
      const int room = cap > 0 ? cap : 1;
      mvKeys.resize(room);
      mvKeysUn.resize(room);
      mvuRight.resize(room);
      mvDepth.resize(room);
      cv::Mat desc(room, 32, CV_8U);
      const orbx_camera cam = frame_camera(mK, mDistCoef);
      int n = 0;
      check(orbx_frame_rgbd(ex->gpu(), im.data, im.step, im.cols, im.rows, im.channels(), bRGB ? 1 : 0, imDepth->data,
                            imDepth->step, imDepth->cols, imDepth->rows, imDepth->type(), depthMapFactor, &cam, mbf,
                            reinterpret_cast<orbx_keypoint*>(mvKeys.data()), desc.data, cap, &n,
                            reinterpret_cast<orbx_keypoint*>(mvKeysUn.data()), mvuRight.data(), mvDepth.data()),
            "orbx_frame_rgbd");
      mvKeys.resize(n);
      mvKeysUn.resize(n);
      mvuRight.resize(n);
      mvDepth.resize(n);
      if (n) {  // ExtractForFrame's outputs: exactly n descriptor rows, no pyramid kept
        mDescriptors.create(n, 32, CV_8U);
        std::memcpy(mDescriptors.data, desc.data, (size_t)32 * n);
      }
      for (int l = 0; l < ex->nlevels; l++) ex->mvImagePyramid[l].release();
    }
    N = (int)mvKeys.size();
    if (mvKeys.empty()) return;  // :147-148
  } else {
    ExtractORB(0, im);  // :204
    N = (int)mvKeys.size();
    if (mvKeys.empty()) return;  // :208-209
    UndistortKeyPoints();
    mvuRight.assign(N, -1.0f);  // no stereo information, :215-216
    mvDepth.assign(N, -1.0f);
  }
  mvpMapPoints.assign(N, nullptr);
  mvbOutlier.assign(N, false);
  // only for the first Frame, or after a change in the calibration (:162-177, 223-245)
  if (mbInitialComputations) {
    ComputeImageBounds(im);
    mfGridElementWidthInv = static_cast<float>(ORBX_GRID_COLS) / (mnMaxX - mnMinX);
    mfGridElementHeightInv = static_cast<float>(ORBX_GRID_ROWS) / (mnMaxY - mnMinY);
    fx = mK.at<float>(0, 0);
    fy = mK.at<float>(1, 1);
    cx = mK.at<float>(0, 2);
    cy = mK.at<float>(1, 2);
    invfx = 1.0f / fx;
    invfy = 1.0f / fy;
    mbInitialComputations = false;
  }
  mb = mbf / fx;  // :179, 247
  // AssignFeaturesToGrid (:182, 250): the matchers build the 64x48 grid on the device per call
}

void Frame::ComputeStereoFromRGBD(const cv::Mat& imDepth) {
  // src/Frame.cc:791-816 as written: a float-indexed at<float> truncates, at the distorted keypoint
  if (imDepth.type() != CV_32F) throw std::invalid_argument("Frame::ComputeStereoFromRGBD: imDepth must be CV_32F");
  mvuRight.assign(N, -1.0f);
  mvDepth.assign(N, -1.0f);
  for (int i = 0; i < N; i++) {
    const cv::KeyPoint& kp = mvKeys[i];
    const cv::KeyPoint& kpU = mvKeysUn[i];
    const int v = (int)kp.pt.y, u = (int)kp.pt.x;
    if (v < 0 || v >= imDepth.rows || u < 0 || u >= imDepth.cols)
      throw std::out_of_range("Frame::ComputeStereoFromRGBD: keypoint outside the depth image");
    const float d = imDepth.at<float>(v, u);
    if (d > 0) {
      mvDepth[i] = d;
      mvuRight[i] = kpU.pt.x - mbf / d;
    }
  }
}

}  // namespace ORB_SLAM2

// cv::cvtColor for Tracking::GrabImage*'s four codes (src/Tracking.cc:174-199, 215-228, 246-259)
void cv::cvtColor(cv::InputArray src, cv::OutputArray dst, int code, int) {
  const cv::Mat s = src.getMat();  // shares the data: dst may be the same Mat
  const bool four = code == CV_BGRA2GRAY || code == CV_RGBA2GRAY, rgb = code == CV_RGB2GRAY || code == CV_RGBA2GRAY;
  if (code != CV_BGR2GRAY && code != CV_RGB2GRAY && code != CV_BGRA2GRAY && code != CV_RGBA2GRAY)
    throw std::invalid_argument("cv::cvtColor: only CV_BGR2GRAY, CV_RGB2GRAY, CV_BGRA2GRAY and CV_RGBA2GRAY");
  if (s.type() != (four ? CV_8UC4 : CV_8UC3)) throw std::invalid_argument("cv::cvtColor: source channels do not fit the code");
  cv::Mat g(s.rows, s.cols, CV_8UC1);
  const orbx_status st = orbx_cvt_gray(s.data, s.step, s.step * (size_t)s.rows, 1, s.cols, s.rows, four ? 4 : 3, rgb ? 1 : 0,
                                       g.data, g.step, g.step * (size_t)g.rows, ORB_SLAM2::gOrbxDevice);
  if (st != ORBX_OK) throw std::runtime_error("orbx_cvt_gray failed: orbx_status " + std::to_string(st));
  dst.getMatRef() = g;
}

namespace ORB_SLAM2 {

void Frame::ComputeImageBounds(const cv::Mat& imLeft) {
  // src/Frame.cc:508-537: the undistorted image corners (cv::undistortPoints with P = K on the GPU)
  if (!mDistCoef.empty() && mDistCoef.at<float>(0, 0) != 0.0f) {
    const float cols = (float)imLeft.cols, rows = (float)imLeft.rows;
    std::vector<cv::KeyPoint> corners = {cv::KeyPoint(0.f, 0.f, 1.f), cv::KeyPoint(cols, 0.f, 1.f),
                                         cv::KeyPoint(0.f, rows, 1.f), cv::KeyPoint(cols, rows, 1.f)};
    std::vector<cv::KeyPoint> un(4);
    orbx_camera cam;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) cam.K[3 * r + c] = mK.at<float>(r, c);
    const int nd = mDistCoef.rows * mDistCoef.cols;
    cam.n_dist = nd;
    for (int i = 0; i < 5; i++) cam.dist[i] = i < nd ? mDistCoef.ptr<float>(0)[i] : 0.f;
    check(orbx_undistort_keypoints(reinterpret_cast<const orbx_keypoint*>(corners.data()), 4, &cam,
                                   reinterpret_cast<orbx_keypoint*>(un.data()), gOrbxDevice),
          "orbx_undistort_keypoints");
    mnMinX = std::min(un[0].pt.x, un[2].pt.x);
    mnMaxX = std::max(un[1].pt.x, un[3].pt.x);
    mnMinY = std::min(un[0].pt.y, un[1].pt.y);
    mnMaxY = std::max(un[2].pt.y, un[3].pt.y);
  } else {
    mnMinX = 0.0f;
    mnMaxX = (float)imLeft.cols;
    mnMinY = 0.0f;
    mnMaxY = (float)imLeft.rows;
  }
}

void Frame::SetPose(const cv::Mat& Tcw) {  // src/Frame.cc:287-291
  mTcw = Tcw.clone();
  UpdatePoseMatrices();
}

void Frame::UpdatePoseMatrices() {  // src/Frame.cc:294-304
  mRcw.create(3, 3, CV_32F);
  mRwc.create(3, 3, CV_32F);
  mtcw.create(3, 1, CV_32F);
  mOw.create(3, 1, CV_32F);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {
      mRcw.at<float>(r, c) = mTcw.at<float>(r, c);
      mRwc.at<float>(c, r) = mTcw.at<float>(r, c);
    }
    mtcw.at<float>(r, 0) = mTcw.at<float>(r, 3);
  }
  // mOw = -mRcw.t()*mtcw: one float gemm with alpha = -1, accumulated in double, rounded once
  for (int r = 0; r < 3; r++) {
    double acc = 0.0;
    for (int k = 0; k < 3; k++) acc += (double)mRcw.at<float>(k, r) * (double)mtcw.at<float>(k, 0);
    mOw.at<float>(r, 0) = (float)(-acc);
  }
}

void Frame::ComputeBoW() {  // src/Frame.cc:462-469
  if (mBowVec.empty()) {
    if (!mpORBvocabulary) throw std::runtime_error("Frame::ComputeBoW: no vocabulary");
    mpORBvocabulary->transform(mDescriptors, mBowVec, mFeatVec, 4);
  }
}

void KeyFrame::ComputeBoW() {  // src/KeyFrame.cc:65-80
  if (mBowVec.empty() || mFeatVec.empty()) {
    if (!mpORBvocabulary) throw std::runtime_error("KeyFrame::ComputeBoW: no vocabulary");
    mpORBvocabulary->transform(mDescriptors, mBowVec, mFeatVec, 4);
  }
}

void Frame::ExtractORB(int flag, const cv::Mat& im) {
  if (flag == 0)
    mpORBextractorLeft->ExtractForFrame(im, mvKeys, mDescriptors);
  else
    mpORBextractorRight->ExtractForFrame(im, mvKeysRight, mDescriptorsRight);
}

void Frame::UndistortKeyPoints() {
  // src/Frame.cc:471-506: no distortion -> copy; otherwise cv::undistortPoints with P = K on the GPU
  if (mDistCoef.empty() || mDistCoef.at<float>(0, 0) == 0.0f) {
    mvKeysUn = mvKeys;
    return;
  }
  orbx_camera cam;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) cam.K[3 * r + c] = mK.at<float>(r, c);
  const int nd = mDistCoef.rows * mDistCoef.cols;
  cam.n_dist = nd;
  for (int i = 0; i < 5; i++) cam.dist[i] = i < nd ? mDistCoef.ptr<float>(0)[i] : 0.f;
  mvKeysUn.resize(N);
  check(orbx_undistort_keypoints(reinterpret_cast<const orbx_keypoint*>(mvKeys.data()), N, &cam,
                                 reinterpret_cast<orbx_keypoint*>(mvKeysUn.data()), gOrbxDevice),
        "orbx_undistort_keypoints");
}

void Frame::ComputeStereoMatches() {
  ORB_SLAM2::ComputeStereoMatches(*mpORBextractorLeft, *mpORBextractorRight, mvKeys, mDescriptors, mvKeysRight,
                                  mDescriptorsRight, mbf, mb, mvuRight, mvDepth);
}

void ComputeStereoMatches(ORBextractor& left, ORBextractor& right, const std::vector<cv::KeyPoint>& kpsL,
                          const cv::Mat& descL, const std::vector<cv::KeyPoint>& kpsR, const cv::Mat& descR,
                          float mbf, float mb, std::vector<float>& mvuRight, std::vector<float>& mvDepth) {
  const int N = (int)kpsL.size();
  mvuRight.assign(N, -1.0f);  // src/Frame.cc:549-550
  mvDepth.assign(N, -1.0f);
  if (N == 0) return;
  const cv::Mat dL = continuous(descL), dR = continuous(descR);
  check(orbx_stereo_match(left.gpu(), right.gpu(), reinterpret_cast<const orbx_keypoint*>(kpsL.data()), dL.data, N,
                          reinterpret_cast<const orbx_keypoint*>(kpsR.data()), kpsR.empty() ? nullptr : dR.data,
                          (int)kpsR.size(), mbf, mb, mvuRight.data(), mvDepth.data()),
        "orbx_stereo_match");
}

// ------------------------------------------------------------------ ORBmatcher
const int ORBmatcher::TH_HIGH = 100;
const int ORBmatcher::TH_LOW = 50;
const int ORBmatcher::HISTO_LENGTH = 30;

ORBmatcher::ORBmatcher(float nnratio, bool checkOri) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

int ORBmatcher::DescriptorDistance(const cv::Mat& a, const cv::Mat& b) {
  // src/ORBmatcher.cc:1844-1860: popcount of the 256-bit XOR (the bit-trick sum there is a popcount)
  const uint32_t* pa = a.ptr<uint32_t>();
  const uint32_t* pb = b.ptr<uint32_t>();
  int dist = 0;
  for (int i = 0; i < 8; i++) dist += __builtin_popcount(pa[i] ^ pb[i]);
  return dist;
}

namespace {
// One side of SearchByBoW with the FeatureVector flattened to CSR (ascending node ids = map order).
struct BowSide {
  std::vector<float> angle;
  std::vector<uint8_t> valid;
  std::vector<uint32_t> ids;
  std::vector<int32_t> off, feat;
  cv::Mat desc;
  orbx_bow_side side(int n, bool with_valid) const {
    return orbx_bow_side{n, n ? desc.data : nullptr, angle.data(), with_valid ? valid.data() : nullptr,
                         (int)ids.size(), ids.data(), off.data(), feat.data()};
  }
};

void fill_fv(BowSide& s, const DBoW2::FeatureVector& fv) {
  s.off.push_back(0);
  for (const auto& node : fv) {
    s.ids.push_back(node.first);
    for (unsigned int f : node.second) s.feat.push_back((int32_t)f);
    s.off.push_back((int32_t)s.feat.size());
  }
}

void fill_keyframe(BowSide& s, const KeyFrame* kf, const std::vector<MapPoint*>& mps) {
  const int n = (int)kf->mvKeysUn.size();
  for (int i = 0; i < n; i++) {
    s.angle.push_back(kf->mvKeysUn[i].angle);
    s.valid.push_back(i < (int)mps.size() && mps[i] && !mps[i]->isBad());
  }
  s.desc = continuous(kf->mDescriptors);
  fill_fv(s, kf->mFeatVec);
}
}  // namespace

int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches) {
  const std::vector<MapPoint*> vpMapPointsKF = pKF->GetMapPointMatches();
  vpMapPointMatches.assign(F.N, nullptr);
  BowSide a, b;
  fill_keyframe(a, pKF, vpMapPointsKF);
  for (int i = 0; i < F.N; i++) b.angle.push_back(F.mvKeys[i].angle);  // rot uses F.mvKeys (:272)
  b.desc = continuous(F.mDescriptors);
  fill_fv(b, F.mFeatVec);
  const orbx_bow_side sa = a.side((int)pKF->mvKeysUn.size(), true), sb = b.side(F.N, false);
  std::vector<int32_t> match(F.N > 0 ? F.N : 1, -1);
  int n = 0;
  check(orbx_search_by_bow_kf_f(&sa, &sb, mfNNratio, mbCheckOrientation, match.data(), &n, gOrbxDevice),
        "orbx_search_by_bow_kf_f");
  for (int i = 0; i < F.N; i++)
    if (match[i] >= 0) vpMapPointMatches[i] = vpMapPointsKF[match[i]];
  return n;
}

int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12) {
  const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
  const std::vector<MapPoint*> vpMapPoints2 = pKF2->GetMapPointMatches();
  const int n1 = (int)pKF1->mvKeysUn.size(), n2 = (int)pKF2->mvKeysUn.size();
  vpMatches12.assign(vpMapPoints1.size(), nullptr);  // :603
  BowSide a, b;
  fill_keyframe(a, pKF1, vpMapPoints1);
  fill_keyframe(b, pKF2, vpMapPoints2);
  const orbx_bow_side sa = a.side(n1, true), sb = b.side(n2, true);
  std::vector<int32_t> match(n1 > 0 ? n1 : 1, -1);
  int n = 0;
  check(orbx_search_by_bow_kf_kf(&sa, &sb, mfNNratio, mbCheckOrientation, match.data(), &n, gOrbxDevice),
        "orbx_search_by_bow_kf_kf");
  for (int i = 0; i < n1 && i < (int)vpMatches12.size(); i++)
    if (match[i] >= 0) vpMatches12[i] = vpMapPoints2[match[i]];
  return n;
}

// ------------------------------------------------------------------ SearchByProjection / Fuse
namespace {
// mvpMapPoints on entry, as the kernel reads it: 0 NULL, 1 a MapPoint with Observations() == 0,
// 2 a MapPoint with Observations() > 0 (the reference's "F.mvpMapPoints[idx]->Observations() > 0")
int8_t occupancy(MapPoint* p) { return !p ? 0 : (p->Observations() > 0 ? 2 : 1); }

void copy_desc(MapPoint* p, uint8_t* dst) {
  const cv::Mat d = p->GetDescriptor();
  if (d.empty())
    std::memset(dst, 0, 32);
  else
    std::memcpy(dst, d.ptr<uint8_t>(0), 32);
}

void copy_pos(MapPoint* p, float* dst) {
  const cv::Mat X = p->GetWorldPos();
  for (int k = 0; k < 3; k++) dst[k] = X.at<float>(k, 0);
}

void copy_dist(MapPoint* p, float* dst) {  // mfMinDistance, mfMaxDistance (the kernel applies 0.8 / 1.2)
  std::unique_lock<std::mutex> lock(p->mMutexPos);
  dst[0] = p->mfMinDistance;
  dst[1] = p->mfMaxDistance;
}

void copy_mat44(const cv::Mat& T, float* dst) {
  for (int i = 0; i < 16; i++) dst[i] = (i < 12 || T.rows == 4) ? T.at<float>(i / 4, i % 4) : (i == 15 ? 1.f : 0.f);
}

void set_levels(orbx_proj_frame& f, int nlevels, const std::vector<float>& sf, const std::vector<float>& isig) {
  if (nlevels < 1 || nlevels > 16 || (int)sf.size() < nlevels) throw std::invalid_argument("orbx shim: nlevels");
  f.nlevels = nlevels;
  for (int l = 0; l < 16; l++) {
    f.scale_factors[l] = l < nlevels ? sf[l] : 0.f;
    f.inv_level_sigma2[l] = l < nlevels && l < (int)isig.size() ? isig[l] : 0.f;
  }
}

// The current Frame as orbx_proj_frame (pointers into F and into the caller's occ / desc buffers)
orbx_proj_frame proj_frame(Frame& F, std::vector<int8_t>& occ, cv::Mat& desc) {
  orbx_proj_frame f;
  std::memset(&f, 0, sizeof(f));
  f.n = F.N;
  occ.resize(F.N > 0 ? F.N : 1);
  for (int i = 0; i < F.N; i++) occ[i] = occupancy(F.mvpMapPoints[i]);
  desc = continuous(F.mDescriptors);
  f.keys_un = reinterpret_cast<const orbx_keypoint*>(F.mvKeysUn.data());
  f.desc = F.N > 0 ? desc.data : nullptr;
  f.u_right = F.mvuRight.empty() ? nullptr : F.mvuRight.data();
  f.occ = occ.data();
  f.min_x = Frame::mnMinX;
  f.max_x = Frame::mnMaxX;
  f.min_y = Frame::mnMinY;
  f.max_y = Frame::mnMaxY;
  f.grid_inv_w = Frame::mfGridElementWidthInv;
  f.grid_inv_h = Frame::mfGridElementHeightInv;
  set_levels(f, F.mnScaleLevels, F.mvScaleFactors, F.mvInvLevelSigma2);
  f.log_scale_factor = F.mfLogScaleFactor;
  f.fx = Frame::fx;
  f.fy = Frame::fy;
  f.cx = Frame::cx;
  f.cy = Frame::cy;
  f.bf = F.mbf;
  f.b = F.mb;
  copy_mat44(F.mTcw, f.Tcw);
  return f;
}

// The projected MapPoints of one call, SoA
struct ProjPoints {
  std::vector<uint8_t> desc, flags;
  std::vector<float> pos, normal, dist, angle, track;
  std::vector<int32_t> octave, level, point_match;
  explicit ProjPoints(size_t n)
      : desc(32 * std::max<size_t>(n, 1), 0), flags(std::max<size_t>(n, 1), 0), pos(3 * std::max<size_t>(n, 1), 0.f),
        normal(3 * std::max<size_t>(n, 1), 0.f), dist(2 * std::max<size_t>(n, 1), 0.f),
        angle(std::max<size_t>(n, 1), 0.f), track(4 * std::max<size_t>(n, 1), 0.f),
        octave(std::max<size_t>(n, 1), 0), level(std::max<size_t>(n, 1), 0), point_match(std::max<size_t>(n, 1), -1) {}
  void fill(orbx_proj_problem& p, int n) {
    p.n_points = n;
    p.desc = desc.data();
    p.flags = flags.data();
    p.pos = pos.data();
    p.normal = normal.data();
    p.dist_minmax = dist.data();
    p.angle = angle.data();
    p.octave = octave.data();
    p.track = track.data();
    p.track_level = level.data();
    p.point_match = point_match.data();
  }
};

orbx_proj_problem proj_problem(int kind, float th, const ORBmatcher& m) {
  orbx_proj_problem p;
  std::memset(&p, 0, sizeof(p));
  p.kind = kind;
  p.th = th;
  p.view_cos_limit = 0.5f;
  (void)m;
  return p;
}

// frame_out -> the Frame's mvpMapPoints, as the reference's assignments leave them
void apply_frame_out(Frame& F, const std::vector<int32_t>& frame_out, const std::vector<MapPoint*>& pts) {
  for (int i = 0; i < F.N; i++) {
    const int k = frame_out[i];
    if (k >= 0)
      F.mvpMapPoints[i] = pts[k];
    else if (k == -2)
      F.mvpMapPoints[i] = nullptr;
  }
}
}  // namespace

int ORBmatcher::SearchByProjection(Frame& F, const std::vector<MapPoint*>& vpMapPoints, const float th) {
  // src/ORBmatcher.cc:46-142.  The MapPoints carry Tracking::SearchLocalPoints' frustum results
  // (mbTrackInView, mTrackProjX/Y/XR, mnTrackScaleLevel, mTrackViewCos).
  const int n = (int)vpMapPoints.size();
  std::vector<int8_t> occ;
  cv::Mat desc;
  orbx_proj_problem p = proj_problem(ORBX_PROJ_LOCAL, th, *this);
  p.f = proj_frame(F, occ, desc);
  ProjPoints P(n);
  for (int k = 0; k < n; k++) {
    MapPoint* pMP = vpMapPoints[k];
    if (!pMP) continue;
    const bool take = pMP->mbTrackInView && !pMP->isBad();
    P.flags[k] = (uint8_t)((take ? 1 : 0) | (pMP->Observations() > 0 ? 2 : 0));
    if (!take) continue;
    copy_desc(pMP, &P.desc[32 * (size_t)k]);
    P.track[4 * k] = pMP->mTrackProjX;
    P.track[4 * k + 1] = pMP->mTrackProjY;
    P.track[4 * k + 2] = pMP->mTrackProjXR;
    P.track[4 * k + 3] = pMP->mTrackViewCos;
    P.level[k] = pMP->mnTrackScaleLevel;
  }
  P.fill(p, n);
  p.frustum = 0;
  p.nnratio = mfNNratio;
  p.check_ori = mbCheckOrientation;
  std::vector<int32_t> frame_out(F.N > 0 ? F.N : 1, -1);
  int32_t nm = 0;
  p.frame_out = frame_out.data();
  p.nmatches = &nm;
  check(orbx_search_by_projection(&p, gOrbxDevice), "orbx_search_by_projection");
  apply_frame_out(F, frame_out, vpMapPoints);
  return nm;
}

int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono) {
  // src/ORBmatcher.cc:1489-1646: the last frame's non-outlier MapPoints
  const int n = LastFrame.N;
  std::vector<int8_t> occ;
  cv::Mat desc;
  orbx_proj_problem p = proj_problem(ORBX_PROJ_LAST_FRAME, th, *this);
  p.f = proj_frame(CurrentFrame, occ, desc);
  ProjPoints P(n);
  for (int i = 0; i < n; i++) {
    MapPoint* pMP = LastFrame.mvpMapPoints[i];
    if (!pMP) continue;
    const bool take = !LastFrame.mvbOutlier[i];
    P.flags[i] = (uint8_t)((take ? 1 : 0) | (pMP->Observations() > 0 ? 2 : 0));
    if (!take) continue;
    copy_desc(pMP, &P.desc[32 * (size_t)i]);
    copy_pos(pMP, &P.pos[3 * (size_t)i]);
    P.angle[i] = LastFrame.mvKeysUn[i].angle;
    P.octave[i] = LastFrame.mvKeys[i].octave;
  }
  P.fill(p, n);
  p.check_ori = mbCheckOrientation;
  p.mono = bMono;
  copy_mat44(LastFrame.mTcw, p.last_Tcw);
  std::vector<int32_t> frame_out(CurrentFrame.N > 0 ? CurrentFrame.N : 1, -1);
  int32_t nm = 0;
  p.frame_out = frame_out.data();
  p.nmatches = &nm;
  check(orbx_search_by_projection(&p, gOrbxDevice), "orbx_search_by_projection");
  apply_frame_out(CurrentFrame, frame_out, LastFrame.mvpMapPoints);
  return nm;
}

int ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const std::set<MapPoint*>& sAlreadyFound,
                                   const float th, const int ORBdist) {
  // src/ORBmatcher.cc:1648-1795: the KeyFrame's MapPoints not found yet
  const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
  const int n = (int)vpMPs.size();
  std::vector<int8_t> occ;
  cv::Mat desc;
  orbx_proj_problem p = proj_problem(ORBX_PROJ_KEYFRAME, th, *this);
  p.f = proj_frame(CurrentFrame, occ, desc);
  ProjPoints P(n);
  for (int i = 0; i < n; i++) {
    MapPoint* pMP = vpMPs[i];
    if (!pMP) continue;
    const bool take = !pMP->isBad() && !sAlreadyFound.count(pMP);
    P.flags[i] = (uint8_t)((take ? 1 : 0) | (pMP->Observations() > 0 ? 2 : 0));
    if (!take) continue;
    copy_desc(pMP, &P.desc[32 * (size_t)i]);
    copy_pos(pMP, &P.pos[3 * (size_t)i]);
    copy_dist(pMP, &P.dist[2 * (size_t)i]);
    P.angle[i] = pKF->mvKeysUn[i].angle;
  }
  P.fill(p, n);
  p.check_ori = mbCheckOrientation;
  p.orb_dist = ORBdist;
  std::vector<int32_t> frame_out(CurrentFrame.N > 0 ? CurrentFrame.N : 1, -1);
  int32_t nm = 0;
  p.frame_out = frame_out.data();
  p.nmatches = &nm;
  check(orbx_search_by_projection(&p, gOrbxDevice), "orbx_search_by_projection");
  apply_frame_out(CurrentFrame, frame_out, vpMPs);
  return nm;
}

namespace {
// pKF as the frame of a Fuse problem: its keypoints, descriptors, mvuRight, its own (integer) image
// bounds and grid, scale tables and pose (src/ORBmatcher.cc:918-1054 reads exactly these)
orbx_proj_frame fuse_frame(KeyFrame* pKF, cv::Mat& desc) {
  orbx_proj_frame f;
  std::memset(&f, 0, sizeof(f));
  f.n = pKF->N;
  desc = continuous(pKF->mDescriptors);
  f.keys_un = reinterpret_cast<const orbx_keypoint*>(pKF->mvKeysUn.data());
  f.desc = pKF->N > 0 ? desc.data : nullptr;
  f.u_right = pKF->mvuRight.empty() ? nullptr : pKF->mvuRight.data();
  f.occ = nullptr;
  f.min_x = (float)pKF->mnMinX;
  f.max_x = (float)pKF->mnMaxX;
  f.min_y = (float)pKF->mnMinY;
  f.max_y = (float)pKF->mnMaxY;
  f.grid_inv_w = pKF->mfGridElementWidthInv;
  f.grid_inv_h = pKF->mfGridElementHeightInv;
  // mGrid came from the Frame (KeyFrame.cc constructor), built with the float Frame::mnMinX/mnMinY;
  // the KeyFrame's own (integer) copies above give GetFeaturesInArea's cell range and IsInImage
  f.grid_min_x = Frame::mnMinX;
  f.grid_min_y = Frame::mnMinY;
  f.grid_min_set = 1;
  set_levels(f, pKF->mnScaleLevels, pKF->mvScaleFactors, pKF->mvInvLevelSigma2);
  f.log_scale_factor = pKF->mfLogScaleFactor;
  f.fx = pKF->fx;
  f.fy = pKF->fy;
  f.cx = pKF->cx;
  f.cy = pKF->cy;
  f.bf = pKF->mbf;
  f.b = pKF->mb;
  copy_mat44(pKF->GetPose(), f.Tcw);
  return f;
}

// The matching half of Fuse for the points `which` (indices into vpMapPoints) in their current state:
// best[k] = pKF feature for which[k], or -1
void fuse_match(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, const std::vector<int>& which, float th,
                int device, std::vector<int32_t>& best) {
  const int n = (int)which.size();
  cv::Mat desc;
  orbx_proj_problem p;
  std::memset(&p, 0, sizeof(p));
  p.kind = ORBX_PROJ_FUSE;
  p.th = th;
  p.f = fuse_frame(pKF, desc);
  ProjPoints P(n);
  for (int k = 0; k < n; k++) {
    MapPoint* pMP = vpMapPoints[which[k]];
    if (!pMP) continue;
    const bool take = !pMP->isBad() && !pMP->IsInKeyFrame(pKF);
    P.flags[k] = (uint8_t)((take ? 1 : 0) | (pMP->Observations() > 0 ? 2 : 0));
    if (!take) continue;
    copy_desc(pMP, &P.desc[32 * (size_t)k]);
    copy_pos(pMP, &P.pos[3 * (size_t)k]);
    const cv::Mat nrm = pMP->GetNormal();
    for (int c = 0; c < 3; c++) P.normal[3 * (size_t)k + c] = nrm.empty() ? 0.f : nrm.at<float>(c, 0);
    copy_dist(pMP, &P.dist[2 * (size_t)k]);
  }
  P.fill(p, n);
  std::vector<int32_t> frame_out(pKF->N > 0 ? pKF->N : 1, -1);
  int32_t nm = 0;
  p.frame_out = frame_out.data();
  p.nmatches = &nm;
  check(orbx_search_by_projection(&p, device), "orbx_search_by_projection (Fuse)");
  best.assign(P.point_match.begin(), P.point_match.begin() + n);
}
}  // namespace

int ORBmatcher::Fuse(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, const float th) {
  // src/ORBmatcher.cc:918-1092.  Point i's match depends only on point i and pKF's keypoints, so all
  // points are matched in one launch on their entry state; the Replace / AddObservation block then
  // runs here in point order, as the reference's loop does.  A later point whose own state an
  // earlier Replace changed (it received observations and a new descriptor, or became bad) is
  // matched again in its current state before it is applied.
  const int n = (int)vpMapPoints.size();
  std::vector<int> all(n);
  for (int i = 0; i < n; i++) all[i] = i;
  std::vector<int32_t> best;
  fuse_match(pKF, vpMapPoints, all, th, gOrbxDevice, best);
  std::set<MapPoint*> touched;  // MapPoints an earlier Replace modified
  int nFused = 0;
  for (int i = 0; i < n; i++) {
    MapPoint* pMP = vpMapPoints[i];
    if (!pMP) continue;
    int bestIdx = best[i];
    if (touched.count(pMP)) {
      std::vector<int32_t> b1;
      fuse_match(pKF, vpMapPoints, std::vector<int>{i}, th, gOrbxDevice, b1);
      bestIdx = b1[0];
    }
    if (bestIdx < 0) continue;
    if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;  // the reference's check, at this point's turn
    MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
    if (pMPinKF) {
      if (!pMPinKF->isBad()) {
        if (pMPinKF->Observations() > pMP->Observations()) {
          pMP->Replace(pMPinKF);
          touched.insert(pMPinKF);
        } else {
          pMPinKF->Replace(pMP);
          touched.insert(pMP);
        }
        touched.insert(pMP);
        touched.insert(pMPinKF);
      }
    } else {
      pMP->AddObservation(pKF, bestIdx);
      pKF->AddMapPoint(pMP, bestIdx);
      touched.insert(pMP);
    }
    nFused++;
  }
  return nFused;
}

int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*>& vpPoints,
                                   std::vector<MapPoint*>& vpMatched, int th) {
  // src/ORBmatcher.cc:327-440 (caller LoopClosing::ComputeSim3, src/LoopClosing.cc:504): one
  // ORBX_PROJ_SIM3 problem; vpMatched on entry blocks its features (occ) and its MapPoints
  // (spAlreadyFound), the kernel's sweeps reproduce the in-order "vpMatched[idx]" skips
  const int n = (int)vpPoints.size();
  cv::Mat desc;
  orbx_proj_problem p;
  std::memset(&p, 0, sizeof(p));
  p.kind = ORBX_PROJ_SIM3;
  p.th = (float)th;
  p.f = fuse_frame(pKF, desc);
  copy_mat44(Scw, p.f.Tcw);
  std::vector<int8_t> occ(pKF->N > 0 ? pKF->N : 1, 0);
  std::set<MapPoint*> found;
  for (int i = 0; i < pKF->N && i < (int)vpMatched.size(); i++)
    if (vpMatched[i]) {
      occ[i] = 1;
      found.insert(vpMatched[i]);
    }
  p.f.occ = occ.data();
  ProjPoints P(n);
  for (int k = 0; k < n; k++) {
    MapPoint* pMP = vpPoints[k];
    if (!pMP || pMP->isBad() || found.count(pMP)) continue;
    P.flags[k] = 1;
    copy_desc(pMP, &P.desc[32 * (size_t)k]);
    copy_pos(pMP, &P.pos[3 * (size_t)k]);
    const cv::Mat nrm = pMP->GetNormal();
    for (int c = 0; c < 3; c++) P.normal[3 * (size_t)k + c] = nrm.empty() ? 0.f : nrm.at<float>(c, 0);
    copy_dist(pMP, &P.dist[2 * (size_t)k]);
  }
  P.fill(p, n);
  std::vector<int32_t> frame_out(pKF->N > 0 ? pKF->N : 1, -1);
  int32_t nm = 0;
  p.frame_out = frame_out.data();
  p.nmatches = &nm;
  check(orbx_search_by_projection(&p, gOrbxDevice), "orbx_search_by_projection (Sim3)");
  for (int i = 0; i < pKF->N && i < (int)vpMatched.size(); i++)
    if (frame_out[i] >= 0) vpMatched[i] = vpPoints[frame_out[i]];
  return nm;
}

int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, std::vector<cv::Point2f>& vbPrevMatched,
                                        std::vector<int>& vnMatches12, int windowSize) {
  // src/ORBmatcher.cc:442-587 (caller Tracking::MonocularInitialization, src/Tracking.cc:711)
  std::vector<int8_t> occ1, occ2;
  cv::Mat d1, d2;
  orbx_init_problem p;
  std::memset(&p, 0, sizeof(p));
  p.f1 = proj_frame(F1, occ1, d1);
  p.f2 = proj_frame(F2, occ2, d2);
  const int n1 = F1.N;
  std::vector<float> prev(2 * (size_t)(n1 > 0 ? n1 : 1), 0.f);
  for (int i = 0; i < n1 && i < (int)vbPrevMatched.size(); i++) {
    prev[2 * i] = vbPrevMatched[i].x;
    prev[2 * i + 1] = vbPrevMatched[i].y;
  }
  std::vector<int32_t> m(n1 > 0 ? n1 : 1, -1);
  int32_t nm = 0;
  p.prev_matched = prev.data();
  p.window = windowSize;
  p.nnratio = mfNNratio;
  p.check_ori = mbCheckOrientation ? 1 : 0;
  p.match12 = m.data();
  p.nmatches = &nm;
  check(orbx_search_for_initialization(&p, gOrbxDevice), "orbx_search_for_initialization");
  vnMatches12.assign(m.begin(), m.begin() + n1);
  for (int i = 0; i < n1 && i < (int)vbPrevMatched.size(); i++)
    if (m[i] >= 0) vbPrevMatched[i] = cv::Point2f(prev[2 * i], prev[2 * i + 1]);
  return nm;
}

int ORBmatcher::SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, const float& s12,
                             const cv::Mat& R12, const cv::Mat& t12, const float th) {
  // src/ORBmatcher.cc:1238-1487 (caller LoopClosing::ComputeSim3, src/LoopClosing.cc:422): both
  // directions on the GPU (orbx_search_by_sim3), vbAlreadyMatched1/2 from vpMatches12 here (:1262-1273)
  const std::vector<MapPoint*> vp1 = pKF1->GetMapPointMatches(), vp2 = pKF2->GetMapPointMatches();
  const int N1 = (int)vp1.size(), N2 = (int)vp2.size();
  std::vector<char> am1(N1, 0), am2(N2, 0);
  for (int i = 0; i < N1 && i < (int)vpMatches12.size(); i++) {
    MapPoint* pMP = vpMatches12[i];
    if (!pMP) continue;
    am1[i] = 1;
    const int idx2 = pMP->GetIndexInKeyFrame(pKF2);
    if (idx2 >= 0 && idx2 < N2) am2[idx2] = 1;
  }
  orbx_sim3_problem p;
  std::memset(&p, 0, sizeof(p));
  cv::Mat d1, d2;
  p.kf1 = fuse_frame(pKF1, d1);
  p.kf2 = fuse_frame(pKF2, d2);
  ProjPoints P1(N1), P2(N2);
  auto side = [](const std::vector<MapPoint*>& vp, const std::vector<char>& am, ProjPoints& P) {
    for (size_t i = 0; i < vp.size(); i++) {
      MapPoint* pMP = vp[i];
      if (!pMP || am[i] || pMP->isBad()) continue;
      P.flags[i] = 1;
      copy_desc(pMP, &P.desc[32 * i]);
      copy_pos(pMP, &P.pos[3 * i]);
      copy_dist(pMP, &P.dist[2 * i]);
    }
  };
  side(vp1, am1, P1);
  side(vp2, am2, P2);
  p.desc1 = P1.desc.data();
  p.pos1 = P1.pos.data();
  p.dist_minmax1 = P1.dist.data();
  p.flags1 = P1.flags.data();
  p.desc2 = P2.desc.data();
  p.pos2 = P2.pos.data();
  p.dist_minmax2 = P2.dist.data();
  p.flags2 = P2.flags.data();
  p.s12 = s12;
  for (int i = 0; i < 9; i++) p.R12[i] = R12.at<float>(i / 3, i % 3);
  for (int i = 0; i < 3; i++) p.t12[i] = t12.at<float>(i, 0);
  p.th = th;
  std::vector<int32_t> m12(N1 > 0 ? N1 : 1, -1);
  int32_t nf = 0;
  p.match12 = m12.data();
  p.nfound = &nf;
  check(orbx_search_by_sim3(&p, gOrbxDevice), "orbx_search_by_sim3");
  for (int i1 = 0; i1 < N1 && i1 < (int)vpMatches12.size(); i1++)
    if (m12[i1] >= 0) vpMatches12[i1] = vp2[m12[i1]];
  return nf;
}

std::set<MapPoint*> KeyFrame::GetMapPoints() {
  std::unique_lock<std::mutex> lock(mMutexFeatures);
  std::set<MapPoint*> s;
  for (MapPoint* pMP : mvpMapPoints)
    if (pMP && !pMP->isBad()) s.insert(pMP);
  return s;
}

int ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*>& vpPoints, float th,
                     std::vector<MapPoint*>& vpReplacePoint) {
  // src/ORBmatcher.cc:1094-1236 (caller LoopClosing::SearchAndFuse, src/LoopClosing.cc:837).  The
  // candidate loop reads no state the loop writes, so every point is matched in one launch
  // (ORBX_PROJ_FUSE_SIM3); the replace / AddMapPoint block then runs here in point order.
  const std::set<MapPoint*> found = pKF->GetMapPoints();
  const int n = (int)vpPoints.size();
  cv::Mat desc;
  orbx_proj_problem p;
  std::memset(&p, 0, sizeof(p));
  p.kind = ORBX_PROJ_FUSE_SIM3;
  p.th = th;
  p.f = fuse_frame(pKF, desc);
  copy_mat44(Scw, p.f.Tcw);
  ProjPoints P(n);
  for (int k = 0; k < n; k++) {
    MapPoint* pMP = vpPoints[k];
    if (!pMP || pMP->isBad() || found.count(pMP)) continue;
    P.flags[k] = 1;
    copy_desc(pMP, &P.desc[32 * (size_t)k]);
    copy_pos(pMP, &P.pos[3 * (size_t)k]);
    const cv::Mat nrm = pMP->GetNormal();
    for (int c = 0; c < 3; c++) P.normal[3 * (size_t)k + c] = nrm.empty() ? 0.f : nrm.at<float>(c, 0);
    copy_dist(pMP, &P.dist[2 * (size_t)k]);
  }
  P.fill(p, n);
  std::vector<int32_t> frame_out(pKF->N > 0 ? pKF->N : 1, -1);
  int32_t nm = 0;
  p.frame_out = frame_out.data();
  p.nmatches = &nm;
  check(orbx_search_by_projection(&p, gOrbxDevice), "orbx_search_by_projection (Fuse Sim3)");
  int nFused = 0;
  for (int i = 0; i < n; i++) {
    const int bestIdx = P.point_match[i];
    if (bestIdx < 0) continue;
    MapPoint* pMP = vpPoints[i];
    MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
    if (pMPinKF) {
      if (!pMPinKF->isBad() && i < (int)vpReplacePoint.size()) vpReplacePoint[i] = pMPinKF;
    } else {
      pMP->AddObservation(pKF, bestIdx);
      pKF->AddMapPoint(pMP, bestIdx);
    }
    nFused++;
  }
  return nFused;
}

int ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat F12,
                                       std::vector<std::pair<size_t, size_t>>& vMatchedPairs, const bool bOnlyStereo) {
  // src/ORBmatcher.cc:738-925 (caller LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:363)
  struct Side {
    std::vector<uint8_t> has_mp;
    std::vector<uint32_t> ids;
    std::vector<int32_t> off, feat;
    cv::Mat desc;
    orbx_tri_kf kf(KeyFrame* K) {
      const int n = K->N;
      has_mp.assign(n > 0 ? n : 1, 0);
      for (int i = 0; i < n; i++) has_mp[i] = K->GetMapPoint(i) != nullptr;
      off.push_back(0);
      for (const auto& node : K->mFeatVec) {
        ids.push_back(node.first);
        for (unsigned int f : node.second) feat.push_back((int32_t)f);
        off.push_back((int32_t)feat.size());
      }
      desc = continuous(K->mDescriptors);
      return orbx_tri_kf{n, reinterpret_cast<const orbx_keypoint*>(K->mvKeysUn.data()), n > 0 ? desc.data : nullptr,
                         K->mvuRight.empty() ? nullptr : K->mvuRight.data(), has_mp.data(), (int)ids.size(),
                         ids.data(), off.data(), feat.data()};
    }
  } s1, s2;
  orbx_tri_problem p;
  std::memset(&p, 0, sizeof(p));
  p.kf1 = s1.kf(pKF1);
  p.kf2 = s2.kf(pKF2);
  for (int i = 0; i < 9; i++) p.F12[i] = F12.at<float>(i / 3, i % 3);
  const cv::Mat C1 = pKF1->GetCameraCenter();
  for (int k = 0; k < 3; k++) p.C1w[k] = C1.at<float>(k, 0);
  copy_mat44(pKF2->GetPose(), p.T2w);
  p.fx = pKF2->fx;
  p.fy = pKF2->fy;
  p.cx = pKF2->cx;
  p.cy = pKF2->cy;
  const int nl = pKF2->mnScaleLevels;
  if (nl < 1 || nl > 16) throw std::invalid_argument("SearchForTriangulation: nlevels");
  for (int l = 0; l < 16; l++) {
    p.scale_factors2[l] = l < nl ? pKF2->mvScaleFactors[l] : 0.f;
    p.level_sigma2_2[l] = l < nl ? pKF2->mvLevelSigma2[l] : 0.f;
  }
  p.only_stereo = bOnlyStereo;
  p.check_ori = mbCheckOrientation;
  std::vector<int32_t> m12(pKF1->N > 0 ? pKF1->N : 1, -1);
  int32_t nm = 0;
  p.match12 = m12.data();
  p.nmatches = &nm;
  check(orbx_search_for_triangulation(&p, gOrbxDevice), "orbx_search_for_triangulation");
  vMatchedPairs.clear();
  vMatchedPairs.reserve(nm);
  for (int i = 0; i < pKF1->N; i++)
    if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));
  return nm;
}

// ------------------------------------------------------------------ LocalMapping::CreateNewMapPoints
LocalMapping::LocalMapping(Map* pMap, const float bMonocular) : mpMap(pMap), mbMonocular(bMonocular != 0.f) {}

LocalMapping::~LocalMapping() {
  if (mpGpu) orbx_new_points_destroy(mpGpu);
}

void LocalMapping::InsertKeyFrame(KeyFrame* pKF) {
  std::unique_lock<std::mutex> lock(mMutexNewKFs);
  mlNewKeyFrames.push_back(pKF);
  mbAbortBA = true;
  if (mpFlag) *mpFlag = 1;
}

bool LocalMapping::CheckNewKeyFrames() {
  std::unique_lock<std::mutex> lock(mMutexNewKFs);
  return !mlNewKeyFrames.empty();
}

void LocalMapping::CreateNewMapPoints() {
  if (!mpGpu) {
    check(orbx_new_points_create(gOrbxDevice, &mpGpu), "orbx_new_points_create");
    check(orbx_new_points_stop_flag(mpGpu, &mpFlag), "orbx_new_points_stop_flag");
  }
  {
    std::unique_lock<std::mutex> lock(mMutexNewKFs);
    *mpFlag = mlNewKeyFrames.empty() ? 0 : 1;
  }
  const int nn = mbMonocular ? 20 : 10;
  const std::vector<KeyFrame*> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
  struct Side {  // one keyframe's arrays, alive for the call
    std::vector<uint8_t> has_mp;
    std::vector<uint32_t> ids;
    std::vector<int32_t> off, feat;
    std::vector<float> xy, pos;
    cv::Mat desc;
    orbx_new_points_kf kf(KeyFrame* K, bool positions) {
      const int n = K->N;
      has_mp.assign(n > 0 ? n : 1, 0);
      pos.assign(3 * (size_t)(n > 0 ? n : 1), 0.f);
      xy.assign(2 * (size_t)(n > 0 ? n : 1), 0.f);
      for (int i = 0; i < n; i++) {
        MapPoint* pMP = K->GetMapPoint(i);
        has_mp[i] = pMP != nullptr;
        if (pMP && positions) {
          const cv::Mat x = pMP->GetWorldPos();
          for (int k = 0; k < 3; k++) pos[3 * i + k] = x.at<float>(k, 0);
        }
        const cv::KeyPoint& kp = (int)K->mvKeys.size() == n ? K->mvKeys[i] : K->mvKeysUn[i];
        xy[2 * i] = kp.pt.x;
        xy[2 * i + 1] = kp.pt.y;
      }
      off.push_back(0);
      for (const auto& node : K->mFeatVec) {
        ids.push_back(node.first);
        for (unsigned int f : node.second) feat.push_back((int32_t)f);
        off.push_back((int32_t)feat.size());
      }
      desc = continuous(K->mDescriptors);
      orbx_new_points_kf o;
      std::memset(&o, 0, sizeof(o));
      o.kf = orbx_tri_kf{n, reinterpret_cast<const orbx_keypoint*>(K->mvKeysUn.data()), n > 0 ? desc.data : nullptr,
                         (int)K->mvuRight.size() == n && n > 0 ? K->mvuRight.data() : nullptr, has_mp.data(),
                         (int)ids.size(), ids.data(), off.data(), feat.data()};
      o.keys_xy = xy.data();
      o.depth = (int)K->mvDepth.size() == n && n > 0 ? K->mvDepth.data() : nullptr;
      if (o.kf.u_right && !o.depth) throw std::invalid_argument("CreateNewMapPoints: mvuRight without mvDepth");
      o.mp_pos = pos.data();
      copy_mat44(K->GetPose(), o.Tcw);
      o.fx = K->fx, o.fy = K->fy, o.cx = K->cx, o.cy = K->cy, o.mb = K->mb, o.mbf = K->mbf;
      const int nl = K->mnScaleLevels;
      if (nl < 1 || nl > 16 || (int)K->mvScaleFactors.size() < nl || (int)K->mvLevelSigma2.size() < nl)
        throw std::invalid_argument("CreateNewMapPoints: scale tables");
      o.n_levels = nl;
      for (int l = 0; l < nl; l++) {
        o.scale_factors[l] = K->mvScaleFactors[l];
        o.level_sigma2[l] = K->mvLevelSigma2[l];
      }
      return o;
    }
  };
  std::vector<Side> sides(vpNeighKFs.size() + 1);
  std::vector<orbx_new_points_kf> nb(vpNeighKFs.size() > 0 ? vpNeighKFs.size() : 1);
  orbx_new_points_problem p;
  std::memset(&p, 0, sizeof(p));
  p.current = sides[0].kf(mpCurrentKeyFrame, false);
  for (size_t i = 0; i < vpNeighKFs.size(); i++) nb[i] = sides[i + 1].kf(vpNeighKFs[i], mbMonocular);
  p.n_neighbours = (int)vpNeighKFs.size();
  p.neighbours = nb.data();
  p.monocular = mbMonocular;
  p.scale_factor = mpCurrentKeyFrame->mfScaleFactor;
  const size_t n1 = (size_t)(mpCurrentKeyFrame->N > 0 ? mpCurrentKeyFrame->N : 1), nnb = nb.size();
  int32_t n_new = 0, done = 0;
  std::vector<int32_t> idx(3 * n1), skip(nnb), nm(nnb);
  std::vector<float> pos(3 * n1), normal(3 * n1), dist(2 * n1), base(nnb), med(nnb);
  std::vector<uint8_t> has1(n1);
  const orbx_new_points_result r{&n_new,      &done,      idx.data(),  pos.data(), normal.data(), dist.data(),
                                 skip.data(), nm.data(), base.data(), med.data(), has1.data()};
  check(orbx_create_new_map_points(mpGpu, &p, &r), "orbx_create_new_map_points");
  mnNeighboursDone = done;
  for (int k = 0; k < n_new; k++) {  // :539-553, in the reference's order
    KeyFrame* pKF2 = vpNeighKFs[idx[3 * k]];
    const size_t idx1 = (size_t)idx[3 * k + 1], idx2 = (size_t)idx[3 * k + 2];
    cv::Mat x3D(3, 1, CV_32F);
    for (int c = 0; c < 3; c++) x3D.at<float>(c, 0) = pos[3 * k + c];
    MapPoint* pMP = new MapPoint(x3D, mpCurrentKeyFrame, mpMap);
    pMP->AddObservation(mpCurrentKeyFrame, idx1);
    pMP->AddObservation(pKF2, idx2);
    mpCurrentKeyFrame->AddMapPoint(pMP, idx1);
    pKF2->AddMapPoint(pMP, idx2);
    pMP->ComputeDistinctiveDescriptors();
    pMP->UpdateNormalAndDepth();
    if (mpMap) mpMap->AddMapPoint(pMP);
    mlpRecentAddedMapPoints.push_back(pMP);
  }
}

// ------------------------------------------------------------------ MapPoint / ORBVocabulary
void MapPoint::ComputeDistinctiveDescriptors() {
  // src/MapPoint.cc:249-320: the observed descriptors of non-bad KeyFrames in observation (map)
  // order; the one with the least median distance to the others becomes mDescriptor
  std::map<KeyFrame*, size_t> observations;
  {
    std::unique_lock<std::mutex> lock1(mMutexFeatures);
    if (mbBad) return;
    observations = mObservations;
  }
  if (observations.empty()) return;
  std::vector<uint8_t> desc;
  desc.reserve(32 * observations.size());
  for (const auto& o : observations) {
    KeyFrame* pKF = o.first;
    if (pKF->isBad()) continue;
    const uint8_t* row = pKF->mDescriptors.ptr<uint8_t>((int)o.second);
    desc.insert(desc.end(), row, row + 32);
  }
  if (desc.empty()) return;
  const int32_t off[2] = {0, (int32_t)(desc.size() / 32)};
  int32_t best = -1;
  check(orbx_distinctive_descriptors(desc.data(), off, 1, &best, nullptr, gOrbxDevice), "orbx_distinctive_descriptors");
  if (best < 0) return;
  cv::Mat d(1, 32, CV_8U);
  std::memcpy(d.data, &desc[32 * (size_t)best], 32);
  std::unique_lock<std::mutex> lock(mMutexFeatures);
  mDescriptor = d;
}

// ------------------------------------------------------------------ the covisibility table of a Map
Map::~Map() {
  if (mpCovis) orbx_covis_destroy(mpCovis);
}

orbx_covis* Map::Covisibility() {
  if (!mpCovis) check(orbx_covis_create(gOrbxDevice, &mpCovis), "orbx_covis_create");
  return mpCovis;
}

void Map::UploadCovisibilityRow(KeyFrame* pKF) {
  orbx_covis* h = Covisibility();
  const std::vector<MapPoint*> vpMP = pKF->GetMapPointMatches();
  const size_t n = vpMP.size();
  if (pKF->mvKeysUn.size() < n || pKF->mvuRight.size() < n || pKF->mvDepth.size() < n)
    throw std::runtime_error("Map::UploadCovisibilityRow: mvKeysUn / mvuRight / mvDepth shorter than mvpMapPoints");
  std::vector<int32_t> pid(n), oct(n);
  std::vector<uint8_t> flags(n);
  for (size_t i = 0; i < n; i++) {
    MapPoint* pMP = vpMP[i];
    pid[i] = (pMP && !pMP->isBad()) ? (int32_t)pMP->mnId : -1;
    if (pMP && pMP->mnId >= (1ul << 26)) throw std::runtime_error("Map::UploadCovisibilityRow: MapPoint id beyond 2^26");
    if (pid[i] >= 0) mCovisMPs[pMP->mnId] = pMP;
    oct[i] = pKF->mvKeysUn[i].octave;
    flags[i] = (uint8_t)((pKF->mvuRight[i] >= 0 ? ORBX_COVIS_STEREO : 0) |
                         (!(pKF->mvDepth[i] > pKF->mThDepth || pKF->mvDepth[i] < 0) ? ORBX_COVIS_CLOSE : 0));
  }
  check(orbx_covis_set_keyframe(h, (int64_t)pKF->mnId, (int)n, pid.data(), oct.data(), flags.data()),
        "orbx_covis_set_keyframe");
  mCovisKFs[pKF->mnId] = pKF;
}

void Map::CovisibilityPointsBad(const std::vector<MapPoint*>& vpMP) {
  std::vector<int32_t> ids;
  for (MapPoint* p : vpMP)
    if (p && p->mnId < (1ul << 26)) ids.push_back((int32_t)p->mnId);
  if (ids.empty()) return;
  check(orbx_covis_set_points_bad(Covisibility(), ids.data(), (int)ids.size()), "orbx_covis_set_points_bad");
}

void KeyFrame::UpdateConnections() {
  if (!mpMap) throw std::runtime_error("KeyFrame::UpdateConnections: the keyframe has no Map (mpMap)");
  orbx_covis* h = mpMap->Covisibility();
  const int cap = (int)std::max<size_t>(mpMap->mCovisKFs.size(), 1);
  std::vector<int64_t> ck(cap), ok(cap);
  std::vector<int32_t> cw(cap), ow(cap);
  int nc = 0, no = 0;
  // steps 1 and 2 (src/KeyFrame.cc:373-467) on the MI355X; th = 15 (:424)
  check(orbx_covis_update_connections(h, (int64_t)mnId, 15, ck.data(), cw.data(), cap, &nc, ok.data(), ow.data(), cap,
                                      &no),
        "orbx_covis_update_connections");
  if (nc == 0) return;  // :414
  auto kf = [&](int64_t id) {
    KeyFrame* p = mpMap->CovisibilityKeyFrame((long unsigned int)id);
    if (!p) throw std::runtime_error("KeyFrame::UpdateConnections: the table names a keyframe the Map does not know");
    return p;
  };
  std::map<KeyFrame*, int> KFcounter;
  for (int i = 0; i < nc; i++) KFcounter[kf(ck[i])] = cw[i];
  std::vector<KeyFrame*> vpOrdered(no);
  for (int i = 0; i < no; i++) {
    vpOrdered[i] = kf(ok[i]);
    vpOrdered[i]->AddConnection(this, ow[i]);  // :445, :455
  }
  // step 3 (:470-492)
  std::unique_lock<std::mutex> lockCon(mMutexConnections);
  mConnectedKeyFrameWeights = KFcounter;
  mvpOrderedConnectedKeyFrames = vpOrdered;
  mvOrderedWeights.assign(ow.begin(), ow.begin() + no);
  if (mbFirstConnection && mnId != 0) {
    mpParent = mvpOrderedConnectedKeyFrames.front();
    lockCon.unlock();
    mpParent->AddChild(this);
    mbFirstConnection = false;
  }
}

void KeyFrame::SetBadFlag() {
  std::vector<MapPoint*> before;
  for (MapPoint* p : mvpMapPoints)
    if (p && !p->isBad()) before.push_back(p);
  if (!SetBadFlagHost()) return;
  if (!mpMap || !mpMap->CovisibilityKeyFrame(mnId)) return;
  check(orbx_covis_erase_keyframe(mpMap->Covisibility(), (int64_t)mnId), "orbx_covis_erase_keyframe");
  mpMap->mCovisKFs.erase(mnId);
  std::vector<MapPoint*> bad;
  for (MapPoint* p : before)
    if (p->isBad()) bad.push_back(p);  // nObs <= 2 after this keyframe's observation left (src/MapPoint.cc:132)
  mpMap->CovisibilityPointsBad(bad);
}

void LocalMapping::KeyFrameCulling() {
  const std::vector<KeyFrame*> vpLocalKeyFrames = mpCurrentKeyFrame->GetVectorCovisibleKeyFrames();  // :793
  const int n = (int)vpLocalKeyFrames.size();
  if (n == 0) return;
  orbx_covis* h = mpMap->Covisibility();
  std::vector<int64_t> ids(n);
  std::vector<uint8_t> notErase(n), verdict(n);
  size_t cap = 1;
  for (int c = 0; c < n; c++) {
    ids[c] = (int64_t)vpLocalKeyFrames[c]->mnId;
    notErase[c] = vpLocalKeyFrames[c]->mbNotErase ? 1 : 0;
    cap += vpLocalKeyFrames[c]->mvpMapPoints.size();
  }
  std::vector<int32_t> bad(cap);
  int nBad = 0;
  // :796-870, the candidates judged in order on the MI355X
  check(orbx_covis_cull(h, ids.data(), n, notErase.data(), mbMonocular ? 1 : 0, verdict.data(), bad.data(), (int)cap,
                        &nBad),
        "orbx_covis_cull");
  // :869 per verdict: the object-graph half of SetBadFlag (mbNotErase: mbToBeErased, src/KeyFrame.cc:573-577)
  for (int c = 0; c < n; c++) {
    if (verdict[c] == 0) continue;
    KeyFrame* pKF = vpLocalKeyFrames[c];
    if (pKF->SetBadFlagHost()) mpMap->mCovisKFs.erase(pKF->mnId);
  }
  // the points the table turned bad are the ones EraseObservation turned bad on the objects
  for (int i = 0; i < nBad; i++) {
    MapPoint* pMP = mpMap->CovisibilityMapPoint((long unsigned int)bad[i]);
    if (!pMP) throw std::runtime_error("LocalMapping::KeyFrameCulling: the table names a MapPoint the Map does not know");
    if (!pMP->isBad()) pMP->SetBadFlag();
  }
}

ORBVocabulary::~ORBVocabulary() {
  if (mpScoreDb) orbx_kfdb_destroy(mpScoreDb);
  if (mpGpu) orbx_voc_destroy(mpGpu);
}

namespace {
void bow_arrays(const DBoW2::BowVector& v, std::vector<uint32_t>& words, std::vector<double>& values) {
  words.clear();
  values.clear();
  words.reserve(v.size());
  values.reserve(v.size());
  for (const auto& e : v) {  // std::map: ascending word ids
    words.push_back(e.first);
    values.push_back(e.second);
  }
}
}  // namespace

double ORBVocabulary::score(const DBoW2::BowVector& v1, const DBoW2::BowVector& v2) const {
  if (!mpGpu) throw std::runtime_error("ORBVocabulary::score: no vocabulary loaded");
  std::unique_lock<std::mutex> lock(mMutexScore);
  if (!mpScoreDb) check(orbx_kfdb_create(mpGpu, gOrbxDevice, &mpScoreDb), "orbx_kfdb_create");
  std::vector<uint32_t> w1, w2;
  std::vector<double> x1, x2;
  bow_arrays(v1, w1, x1);
  bow_arrays(v2, w2, x2);
  const int64_t id = 0;
  double s = 0.0;
  check(orbx_kfdb_add(mpScoreDb, id, w2.data(), x2.data(), (int)w2.size()), "orbx_kfdb_add");
  const orbx_status st = orbx_kfdb_score(mpScoreDb, w1.data(), x1.data(), (int)w1.size(), &id, 1, &s);
  check(orbx_kfdb_erase(mpScoreDb, id), "orbx_kfdb_erase");
  check(st, "orbx_kfdb_score");
  return s;
}

// ------------------------------------------------------------------ KeyFrameDatabase
KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary& voc) : mpVoc(&voc) {
  check(orbx_kfdb_create(voc.gpu(), gOrbxDevice, &mpGpu), "orbx_kfdb_create");
}

KeyFrameDatabase::~KeyFrameDatabase() {
  if (mpGpu) orbx_kfdb_destroy(mpGpu);
}

void KeyFrameDatabase::add(KeyFrame* pKF) {
  std::unique_lock<std::mutex> lock(mMutex);
  std::vector<uint32_t> w;
  std::vector<double> x;
  bow_arrays(pKF->mBowVec, w, x);
  check(orbx_kfdb_add(mpGpu, (int64_t)pKF->mnId, w.data(), x.data(), (int)w.size()), "orbx_kfdb_add");
  mKeyFrames[pKF->mnId] = pKF;
}

void KeyFrameDatabase::erase(KeyFrame* pKF) {
  std::unique_lock<std::mutex> lock(mMutex);
  check(orbx_kfdb_erase(mpGpu, (int64_t)pKF->mnId), "orbx_kfdb_erase");
  mKeyFrames.erase(pKF->mnId);
}

void KeyFrameDatabase::clear() {
  std::unique_lock<std::mutex> lock(mMutex);
  check(orbx_kfdb_clear(mpGpu), "orbx_kfdb_clear");
  mKeyFrames.clear();
}

void KeyFrameDatabase::UploadNeighbours() {
  const size_t n = mKeyFrames.size();
  std::vector<int64_t> ids(n), best(10 * n, 0);
  std::vector<int32_t> nb(n);
  size_t i = 0;
  for (const auto& e : mKeyFrames) {
    ids[i] = (int64_t)e.first;
    const std::vector<KeyFrame*> vpNeighs = e.second->GetBestCovisibilityKeyFrames(10);
    nb[i] = (int32_t)vpNeighs.size();
    for (size_t j = 0; j < vpNeighs.size(); j++) best[10 * i + j] = (int64_t)vpNeighs[j]->mnId;
    i++;
  }
  check(orbx_kfdb_set_neighbours(mpGpu, ids.data(), best.data(), nb.data(), (int)n), "orbx_kfdb_set_neighbours");
}

void KeyFrameDatabase::WriteBackState() {
  const size_t n = mKeyFrames.size();
  if (!n) return;
  std::vector<int64_t> ids(n);
  std::vector<uint64_t> rq(n), lq(n);
  std::vector<int32_t> rw(n), lw(n);
  std::vector<float> rs(n), ls(n);
  size_t i = 0;
  for (const auto& e : mKeyFrames) ids[i++] = (int64_t)e.first;
  check(orbx_kfdb_read_state(mpGpu, ids.data(), (int)n, rq.data(), rw.data(), rs.data(), lq.data(), lw.data(),
                             ls.data()),
        "orbx_kfdb_read_state");
  i = 0;
  for (const auto& e : mKeyFrames) {
    KeyFrame* pKF = e.second;
    pKF->mnRelocQuery = rq[i];
    pKF->mnRelocWords = rw[i];
    pKF->mRelocScore = rs[i];
    pKF->mnLoopQuery = lq[i];
    pKF->mnLoopWords = lw[i];
    pKF->mLoopScore = ls[i];
    i++;
  }
}

std::vector<KeyFrame*> KeyFrameDatabase::ToKeyFrames(const std::vector<int64_t>& ids) const {
  std::vector<KeyFrame*> out;
  out.reserve(ids.size());
  for (int64_t id : ids) out.push_back(mKeyFrames.at((long unsigned int)id));
  return out;
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame* F) {
  std::unique_lock<std::mutex> lock(mMutex);
  UploadNeighbours();
  std::vector<uint32_t> w;
  std::vector<double> x;
  bow_arrays(F->mBowVec, w, x);
  std::vector<int64_t> cand(std::max<size_t>(mKeyFrames.size(), 1));
  int n = 0;
  check(orbx_kfdb_reloc_candidates(mpGpu, (uint64_t)F->mnId, w.data(), x.data(), (int)w.size(), cand.data(),
                                   (int)cand.size(), &n),
        "orbx_kfdb_reloc_candidates");
  cand.resize(n);
  WriteBackState();
  return ToKeyFrames(cand);
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectLoopCandidates(KeyFrame* pKF, float minScore) {
  const std::set<KeyFrame*> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
  std::unique_lock<std::mutex> lock(mMutex);
  UploadNeighbours();
  std::vector<int64_t> conn;
  conn.reserve(spConnectedKeyFrames.size());
  for (KeyFrame* c : spConnectedKeyFrames) conn.push_back((int64_t)c->mnId);
  std::vector<uint32_t> w;
  std::vector<double> x;
  bow_arrays(pKF->mBowVec, w, x);
  std::vector<int64_t> cand(std::max<size_t>(mKeyFrames.size(), 1));
  int n = 0;
  check(orbx_kfdb_loop_candidates(mpGpu, (uint64_t)pKF->mnId, w.data(), x.data(), (int)w.size(), conn.data(),
                                  (int)conn.size(), minScore, cand.data(), (int)cand.size(), &n),
        "orbx_kfdb_loop_candidates");
  cand.resize(n);
  WriteBackState();
  return ToKeyFrames(cand);
}

bool ORBVocabulary::loadFromText(const std::string& text) {
  if (mpScoreDb) {
    orbx_kfdb_destroy(mpScoreDb);
    mpScoreDb = nullptr;
  }
  if (mpGpu) {
    orbx_voc_destroy(mpGpu);
    mpGpu = nullptr;
  }
  check(orbx_voc_load_text(text.data(), text.size(), gOrbxDevice, &mpGpu), "orbx_voc_load_text");
  check(orbx_voc_info(mpGpu, mInfo), "orbx_voc_info");
  return true;
}

bool ORBVocabulary::loadFromTextFile(const std::string& filename) {
  std::ifstream f(filename.c_str(), std::ios::binary);
  if (!f.is_open()) return false;  // TemplatedVocabulary.h:1343-1347
  std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  return loadFromText(text);
}

void ORBVocabulary::transform(const cv::Mat& descriptors, DBoW2::BowVector& v, DBoW2::FeatureVector& fv,
                              int levelsup) const {
  // TemplatedVocabulary.h:1125-1196 on the device: every row descends the tree there
  v.clear();
  fv.clear();
  if (!mpGpu) throw std::runtime_error("ORBVocabulary::transform: no vocabulary loaded");
  const int n = descriptors.empty() ? 0 : descriptors.rows;
  if (n == 0) return;
  const cv::Mat d = continuous(descriptors);
  const int32_t set_off[2] = {0, n};
  std::vector<uint32_t> words(n), nodes(n);
  std::vector<double> values(n);
  std::vector<int32_t> fv_off(n + 1), fv_feat(n);
  int32_t nb = 0, nf = 0;
  check(orbx_voc_transform(mpGpu, d.data, set_off, 1, levelsup, words.data(), values.data(), &nb, nodes.data(),
                           fv_off.data(), fv_feat.data(), &nf),
        "orbx_voc_transform");
  for (int k = 0; k < nb; k++) v.emplace_hint(v.end(), words[k], values[k]);
  for (int j = 0; j < nf; j++) {
    std::vector<unsigned int>& feats = fv[nodes[j]];
    for (int q = fv_off[j]; q < fv_off[j + 1]; q++) feats.push_back((unsigned int)fv_feat[q]);
  }
}

void ORBVocabulary::transform(const std::vector<cv::Mat>& features, DBoW2::BowVector& v, DBoW2::FeatureVector& fv,
                              int levelsup) const {
  cv::Mat d((int)features.size(), 32, CV_8U);
  for (size_t i = 0; i < features.size(); i++) std::memcpy(d.ptr<uint8_t>((int)i), features[i].ptr<uint8_t>(0), 32);
  if (features.empty()) d.release();
  transform(d, v, fv, levelsup);
}

// ------------------------------------------------------------------ PnPsolver

namespace {
// the process-wide stream DUtils::Random::RandomInt draws from (glibc rand(), seed 1)
std::mutex g_rand_mu;
orbx_rand_state g_rand = [] {
  orbx_rand_state s;
  orbx_rand_seed(&s, 1);
  return s;
}();
}  // namespace

void PnPsolver::SeedRandom(unsigned int seed) {
  std::lock_guard<std::mutex> lock(g_rand_mu);
  orbx_rand_seed(&g_rand, seed);
}

PnPsolver::PnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches)
    : mvpMapPointMatches(vpMapPointMatches) {
  // src/PnPsolver.cc:67-125: one correspondence per matched, non-bad MapPoint, in feature order
  for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
    MapPoint* pMP = vpMapPointMatches[i];
    if (!pMP || pMP->isBad()) continue;
    const cv::KeyPoint& kp = F.mvKeysUn[i];
    mvP2D.push_back(kp.pt.x);
    mvP2D.push_back(kp.pt.y);
    mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
    const cv::Mat Pos = pMP->GetWorldPos();
    for (int k = 0; k < 3; k++) mvP3Dw.push_back(Pos.at<float>(k, 0));
    mvKeyPointIndices.push_back(i);
  }
  fu = F.fx;
  fv = F.fy;
  uc = F.cx;
  vc = F.cy;
  SetRansacParameters();
}

PnPsolver::~PnPsolver() {
  if (mpGpu) orbx_pnp_destroy(mpGpu);
}

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon,
                                    float th2) {
  mParams = orbx_pnp_params{probability, minInliers, maxIterations, minSet, epsilon, th2};
  if (mpGpu) {  // a live solver keeps mnIterations and its best set
    check(orbx_pnp_set_ransac_parameters(mpGpu, mvSigma2.data(), &mParams), "orbx_pnp_set_ransac_parameters");
    int mi = 0;
    float eps = 0;
    check(orbx_pnp_get_params(mpGpu, &mi, &mRansacMaxIts, &eps), "orbx_pnp_get_params");
  }
}

void PnPsolver::ensure_solver() {
  if (mpGpu) return;
  const int n = (int)mvSigma2.size();
  const orbx_pnp_problem prob{n, n ? mvP3Dw.data() : nullptr, n ? mvP2D.data() : nullptr,
                              n ? mvSigma2.data() : nullptr, fu, fv, uc, vc};
  check(orbx_pnp_create(&prob, &mParams, gOrbxDevice, &mpGpu), "orbx_pnp_create");
  int mi = 0;
  float eps = 0;
  check(orbx_pnp_get_params(mpGpu, &mi, &mRansacMaxIts, &eps), "orbx_pnp_get_params");
}

cv::Mat PnPsolver::find(std::vector<bool>& vbInliers, int& nInliers) {
  ensure_solver();
  bool bFlag;
  return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);  // src/PnPsolver.cc:181-185
}

cv::Mat PnPsolver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  ensure_solver();
  bNoMore = false;
  vbInliers.clear();
  nInliers = 0;
  const int n = (int)mvSigma2.size();
  std::vector<uint8_t> inl(n > 0 ? n : 1, 0);
  float T[16];
  int no_more = 0, ni = 0, found = 0;
  {
    std::lock_guard<std::mutex> lock(g_rand_mu);
    check(orbx_pnp_iterate_stream(mpGpu, nIterations, &g_rand, &no_more, T, inl.data(), &ni, &found),
          "orbx_pnp_iterate_stream");
  }
  bNoMore = no_more != 0;
  if (!found) return cv::Mat();
  nInliers = ni;
  vbInliers.assign(mvpMapPointMatches.size(), false);  // :261-266 / :283-288
  for (int i = 0; i < n; i++)
    if (inl[i]) vbInliers[mvKeyPointIndices[i]] = true;
  cv::Mat Tcw(4, 4, CV_32F);
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) Tcw.at<float>(r, c) = T[4 * r + c];
  return Tcw;
}

// ------------------------------------------------------------------ Sim3Solver
namespace {
// Rcw*X + tcw on 3x1 CV_32F Mats: cv::gemm(R, X, 1, t, 1) on OpenCV 3.2's small-matrix path -- the
// dot product in float, left to right, then (float)(t0*alpha + c*beta) in double
void mat3x1(const cv::Mat& R, const cv::Mat& t, const cv::Mat& X, float out[3]) {
  for (int r = 0; r < 3; r++) {
    const float t0 = R.at<float>(r, 0) * X.at<float>(0, 0) + R.at<float>(r, 1) * X.at<float>(1, 0) +
                     R.at<float>(r, 2) * X.at<float>(2, 0);
    out[r] = (float)((double)t0 * 1.0 + (double)t.at<float>(r, 0) * 1.0);
  }
}
}  // namespace

Sim3Solver::Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale)
    : mbFixScale(bFixScale) {
  // src/Sim3Solver.cc:37-125
  const std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
  mN1 = (int)vpMatched12.size();
  const cv::Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation();
  const cv::Mat Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
  for (int i1 = 0; i1 < mN1; i1++) {
    if (!vpMatched12[i1]) continue;
    MapPoint* pMP1 = vpKeyFrameMP1[i1];
    MapPoint* pMP2 = vpMatched12[i1];
    if (!pMP1) continue;
    if (pMP1->isBad() || pMP2->isBad()) continue;
    const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
    const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
    if (indexKF1 < 0 || indexKF2 < 0) continue;
    const cv::KeyPoint& kp1 = pKF1->mvKeysUn[indexKF1];
    const cv::KeyPoint& kp2 = pKF2->mvKeysUn[indexKF2];
    mvSigma2_1.push_back(pKF1->mvLevelSigma2[kp1.octave]);
    mvSigma2_2.push_back(pKF2->mvLevelSigma2[kp2.octave]);
    mvnIndices1.push_back(i1);
    float X[3];
    mat3x1(Rcw1, tcw1, pMP1->GetWorldPos(), X);
    mvX3Dc1.insert(mvX3Dc1.end(), X, X + 3);
    mat3x1(Rcw2, tcw2, pMP2->GetWorldPos(), X);
    mvX3Dc2.insert(mvX3Dc2.end(), X, X + 3);
  }
  mK1[0] = pKF1->fx, mK1[1] = pKF1->fy, mK1[2] = pKF1->cx, mK1[3] = pKF1->cy;  // mK's entries
  mK2[0] = pKF2->fx, mK2[1] = pKF2->fy, mK2[2] = pKF2->cx, mK2[3] = pKF2->cy;
  SetRansacParameters();
}

Sim3Solver::~Sim3Solver() {
  if (mpGpu) orbx_sim3_destroy(mpGpu);
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
  mParams = orbx_sim3_params{probability, minInliers, maxIterations};
  if (mpGpu) {  // a live solver: mnIterations back to 0, the best set kept (:150)
    check(orbx_sim3_set_ransac_parameters(mpGpu, &mParams), "orbx_sim3_set_ransac_parameters");
    check(orbx_sim3_get_params(mpGpu, nullptr, &mRansacMaxIts, nullptr, nullptr), "orbx_sim3_get_params");
  }
}

void Sim3Solver::ensure_solver() {
  if (mpGpu) return;
  const int n = (int)mvnIndices1.size();
  const orbx_sim3_solver_problem prob{n,
                                      n ? mvX3Dc1.data() : nullptr,
                                      n ? mvX3Dc2.data() : nullptr,
                                      n ? mvSigma2_1.data() : nullptr,
                                      n ? mvSigma2_2.data() : nullptr,
                                      mK1[0], mK1[1], mK1[2], mK1[3],
                                      mK2[0], mK2[1], mK2[2], mK2[3],
                                      mbFixScale ? 1 : 0};
  check(orbx_sim3_create(&prob, &mParams, gOrbxDevice, &mpGpu), "orbx_sim3_create");
  check(orbx_sim3_get_params(mpGpu, nullptr, &mRansacMaxIts, nullptr, nullptr), "orbx_sim3_get_params");
}

cv::Mat Sim3Solver::find(std::vector<bool>& vbInliers12, int& nInliers) {
  ensure_solver();
  bool bFlag;
  return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);  // src/Sim3Solver.cc:241-245
}

cv::Mat Sim3Solver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  ensure_solver();
  bNoMore = false;
  vbInliers = std::vector<bool>(mN1, false);  // :157
  nInliers = 0;
  const int n = (int)mvnIndices1.size();
  std::vector<uint8_t> inl(n > 0 ? n : 1, 0);
  float T[16];
  int no_more = 0, ni = 0, found = 0;
  {
    std::lock_guard<std::mutex> lock(g_rand_mu);
    check(orbx_sim3_iterate_stream(mpGpu, nIterations, &g_rand, &no_more, T, inl.data(), &ni, &found),
          "orbx_sim3_iterate_stream");
  }
  bNoMore = no_more != 0;
  if (!found) return cv::Mat();
  nInliers = ni;
  for (int i = 0; i < n; i++)
    if (inl[i]) vbInliers[mvnIndices1[i]] = true;  // :226-228
  cv::Mat T12(4, 4, CV_32F);
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) T12.at<float>(r, c) = T[4 * r + c];
  return T12;
}

cv::Mat Sim3Solver::GetEstimatedRotation() {
  ensure_solver();
  float R[9], t[3], s;
  check(orbx_sim3_get_estimate(mpGpu, R, t, &s), "orbx_sim3_get_estimate");
  cv::Mat m(3, 3, CV_32F);
  for (int i = 0; i < 9; i++) m.at<float>(i / 3, i % 3) = R[i];
  return m;
}

cv::Mat Sim3Solver::GetEstimatedTranslation() {
  ensure_solver();
  float R[9], t[3], s;
  check(orbx_sim3_get_estimate(mpGpu, R, t, &s), "orbx_sim3_get_estimate");
  cv::Mat m(3, 1, CV_32F);
  for (int i = 0; i < 3; i++) m.at<float>(i, 0) = t[i];
  return m;
}

float Sim3Solver::GetEstimatedScale() {
  ensure_solver();
  float R[9], t[3], s;
  check(orbx_sim3_get_estimate(mpGpu, R, t, &s), "orbx_sim3_get_estimate");
  return s;
}

// ------------------------------------------------------------------ Initializer
namespace {
bool g_rand_seeded_once = false;  // DUtils::Random::SeedRandOnce's m_already_seeded (guarded by g_rand_mu)
}  // namespace

Initializer::Initializer(const Frame& ReferenceFrame, float sigma, int iterations)
    : mvKeys1(ReferenceFrame.mvKeysUn), mK(ReferenceFrame.mK.clone()), mSigma(sigma), mMaxIterations(iterations) {
  // src/Initializer.cc:40-53
}

Initializer::~Initializer() {
  if (mpGpu) orbx_initializer_destroy(mpGpu);
}

bool Initializer::Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
                             std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated) {
  const int n1 = (int)mvKeys1.size(), n2 = (int)CurrentFrame.mvKeysUn.size();
  if (!mpGpu) {
    if (mK.rows != 3 || mK.cols != 3 || mK.type() != CV_32F) throw std::runtime_error("Initializer: K must be 3x3 CV_32F");
    std::vector<float> k1(2 * (size_t)(n1 > 0 ? n1 : 1));
    for (int i = 0; i < n1; i++) k1[2 * i] = mvKeys1[i].pt.x, k1[2 * i + 1] = mvKeys1[i].pt.y;
    float K[9];
    for (int i = 0; i < 9; i++) K[i] = mK.at<float>(i / 3, i % 3);
    check(orbx_initializer_create(k1.data(), n1, K, mSigma, mMaxIterations, gOrbxDevice, &mpGpu),
          "orbx_initializer_create");
  }
  if ((int)vMatches12.size() != n1) throw std::runtime_error("Initializer: vMatches12 must have one entry per keypoint");
  std::vector<float> k2(2 * (size_t)(n2 > 0 ? n2 : 1));
  for (int i = 0; i < n2; i++) k2[2 * i] = CurrentFrame.mvKeysUn[i].pt.x, k2[2 * i + 1] = CurrentFrame.mvKeysUn[i].pt.y;
  std::vector<int32_t> m(vMatches12.begin(), vMatches12.end());
  std::vector<float> p3d(3 * (size_t)n1);
  std::vector<uint8_t> tri((size_t)n1);
  float R[9], t[3];
  mResult = orbx_initializer_result{};
  {
    std::lock_guard<std::mutex> lock(g_rand_mu);
    if (!g_rand_seeded_once) {  // DUtils::Random::SeedRandOnce(0), src/Initializer.cc:106
      orbx_rand_seed(&g_rand, 0);
      g_rand_seeded_once = true;
    }
    check(orbx_initializer_initialize_stream(mpGpu, k2.data(), n2, m.data(), &g_rand, R, t, p3d.data(), tri.data(),
                                             &mResult),
          "orbx_initializer_initialize_stream");
  }
  if (!mResult.ok) {
    R21.release();
    t21.release();
    return false;
  }
  R21.create(3, 3, CV_32F);
  t21.create(3, 1, CV_32F);
  for (int i = 0; i < 9; i++) R21.at<float>(i / 3, i % 3) = R[i];
  for (int i = 0; i < 3; i++) t21.at<float>(i, 0) = t[i];
  vP3D.resize(n1);
  vbTriangulated.assign(n1, false);
  for (int i = 0; i < n1; i++) {
    vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
    vbTriangulated[i] = tri[i] != 0;
  }
  return true;
}

// ------------------------------------------------------------------ Optimizer
void (*Optimizer::mpfnGatheredHook)(const LocalBAProblem&, const std::vector<KeyFrame*>&) = nullptr;

int Optimizer::PoseOptimization(Frame* pFrame) {
  // src/Optimizer.cc:287-528: one edge per feature with a MapPoint, in feature order (:318-410);
  // mvbOutlier of those features reset to false; below 3 correspondences the pose is left as is
  const int N = pFrame->N;
  std::vector<float> obs, Xw, isig;
  std::vector<int> idx;
  for (int i = 0; i < N; i++) {
    MapPoint* pMP = pFrame->mvpMapPoints[i];
    if (!pMP) continue;
    pFrame->mvbOutlier[i] = false;
    const cv::KeyPoint& kpUn = pFrame->mvKeysUn[i];
    obs.push_back(kpUn.pt.x);
    obs.push_back(kpUn.pt.y);
    obs.push_back(pFrame->mvuRight[i]);  // < 0: EdgeSE3ProjectXYZOnlyPose, else the stereo edge
    const cv::Mat X = pMP->GetWorldPos();
    for (int k = 0; k < 3; k++) Xw.push_back(X.at<float>(k, 0));
    isig.push_back(pFrame->mvInvLevelSigma2[kpUn.octave]);
    idx.push_back(i);
  }
  const int n = (int)idx.size();
  if (n < 3) return 0;  // :424-425
  orbx_pose_problem p;
  std::memset(&p, 0, sizeof(p));
  p.n = n;
  p.obs = obs.data();
  p.Xw = Xw.data();
  p.inv_sigma2 = isig.data();
  p.fx = Frame::fx;
  p.fy = Frame::fy;
  p.cx = Frame::cx;
  p.cy = Frame::cy;
  p.bf = pFrame->mbf;
  copy_mat44(pFrame->mTcw, p.Tcw);
  float T[16];
  std::vector<uint8_t> outlier(n);
  int32_t ngood = 0;
  p.Tcw_out = T;
  p.outlier = outlier.data();
  p.ngood = &ngood;
  check(orbx_pose_optimization(&p, gOrbxDevice), "orbx_pose_optimization");
  for (int k = 0; k < n; k++) pFrame->mvbOutlier[idx[k]] = outlier[k] != 0;
  cv::Mat pose(4, 4, CV_32F);
  for (int i = 0; i < 16; i++) pose.at<float>(i / 4, i % 4) = T[i];
  pFrame->SetPose(pose);
  return ngood;
}

int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12,
                            const float th2, const bool bFixScale) {
  // src/Optimizer.cc:1236-1384: one correspondence per match with both points good and pMP2 observed
  // in pKF2; the camera-frame points through the float small-gemm path Sim3Solver's gather uses
  const cv::Mat R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation();
  const cv::Mat R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
  const int N = (int)vpMatches1.size();
  const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
  std::vector<float> x1, x2, o1, o2, w1, w2;
  std::vector<size_t> vnIndexEdge;
  for (int i = 0; i < N; i++) {
    if (!vpMatches1[i]) continue;
    MapPoint* pMP1 = vpMapPoints1[i];
    MapPoint* pMP2 = vpMatches1[i];
    const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
    if (!pMP1) continue;
    if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
    float X[3];
    mat3x1(R1w, t1w, pMP1->GetWorldPos(), X);
    x1.insert(x1.end(), X, X + 3);
    mat3x1(R2w, t2w, pMP2->GetWorldPos(), X);
    x2.insert(x2.end(), X, X + 3);
    const cv::KeyPoint& kpUn1 = pKF1->mvKeysUn[i];
    o1.push_back(kpUn1.pt.x);
    o1.push_back(kpUn1.pt.y);
    w1.push_back(pKF1->mvInvLevelSigma2[kpUn1.octave]);
    const cv::KeyPoint& kpUn2 = pKF2->mvKeysUn[i2];
    o2.push_back(kpUn2.pt.x);
    o2.push_back(kpUn2.pt.y);
    w2.push_back(pKF2->mvInvLevelSigma2[kpUn2.octave]);
    vnIndexEdge.push_back((size_t)i);
  }
  const int n = (int)vnIndexEdge.size();
  orbx_optimize_sim3_problem p;
  std::memset(&p, 0, sizeof(p));
  p.n = n;
  p.x3dc1 = x1.data();
  p.x3dc2 = x2.data();
  p.obs1 = o1.data();
  p.obs2 = o2.data();
  p.inv_sigma2_1 = w1.data();
  p.inv_sigma2_2 = w2.data();
  p.K1[0] = pKF1->fx, p.K1[1] = pKF1->fy, p.K1[2] = pKF1->cx, p.K1[3] = pKF1->cy;  // mK's entries
  p.K2[0] = pKF2->fx, p.K2[1] = pKF2->fy, p.K2[2] = pKF2->cx, p.K2[3] = pKF2->cy;
  const g2o::Quaterniond& q = g2oS12.rotation();
  const g2o::Vector3d& t = g2oS12.translation();
  const double S[8] = {q.x(), q.y(), q.z(), q.w(), t[0], t[1], t[2], g2oS12.scale()};
  std::memcpy(p.S12, S, sizeof(S));
  p.th2 = th2;
  p.fix_scale = bFixScale ? 1 : 0;
  double So[8];
  std::vector<uint8_t> inlier(n > 0 ? n : 1, 1);
  int32_t n_in = 0, n_bad = 0;
  p.S12_out = So;
  p.inlier = inlier.data();
  p.n_in = &n_in;
  p.n_bad = &n_bad;
  check(orbx_optimize_sim3(&p, gOrbxDevice), "orbx_optimize_sim3");
  for (int k = 0; k < n; k++)
    if (!inlier[k]) vpMatches1[vnIndexEdge[k]] = static_cast<MapPoint*>(NULL);
  if (n - n_bad < 10) return 0;  // :1423-1424: g2oS12 is not written back
  g2oS12 = g2o::Sim3(g2o::Quaterniond(So[3], So[0], So[1], So[2]), g2o::Vector3d{So[4], So[5], So[6]}, So[7]);
  return n_in;
}

void Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF,
                                       const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                                       const std::map<KeyFrame*, std::set<KeyFrame*>>& LoopConnections,
                                       const bool& bFixScale) {
  const auto byId = [](KeyFrame* a, KeyFrame* b) { return a->mnId < b->mnId; };
  // src/Optimizer.cc:913-971: a vertex per keyframe that is not bad, in ascending mnId (g2o's order of
  // the unknowns); vScw from CorrectedSim3 or Sim3(Rcw, tcw, 1.0)
  std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
  std::sort(vpKFs.begin(), vpKFs.end(), byId);
  const std::vector<MapPoint*> vpMPs = pMap->GetAllMapPoints();
  std::vector<KeyFrame*> vertices;
  std::map<KeyFrame*, int> index;
  for (KeyFrame* pKF : vpKFs)
    if (!pKF->isBad()) {
      index[pKF] = (int)vertices.size();
      vertices.push_back(pKF);
    }
  const int n = (int)vertices.size();
  std::vector<int32_t> ids(n);
  std::vector<double> Scw(8 * (size_t)n), Snc(8 * (size_t)n);
  const auto put = [](const g2o::Sim3& S, double* o) {
    const g2o::Quaterniond& q = S.rotation();
    o[0] = q.x(), o[1] = q.y(), o[2] = q.z(), o[3] = q.w();
    for (int k = 0; k < 3; k++) o[4 + k] = S.translation()[k];
    o[7] = S.scale();
  };
  for (int k = 0; k < n; k++) {
    KeyFrame* pKF = vertices[k];
    ids[k] = (int32_t)pKF->mnId;
    LoopClosing::KeyFrameAndPose::const_iterator it = CorrectedSim3.find(pKF);
    if (it != CorrectedSim3.end()) {
      put(it->second, &Scw[8 * (size_t)k]);
    } else {
      const cv::Mat T = pKF->GetPose();
      float Tcw[12];
      for (int i = 0; i < 12; i++) Tcw[i] = T.at<float>(i / 4, i % 4);
      orbx_sim3_from_tcw(Tcw, &Scw[8 * (size_t)k]);
    }
    it = NonCorrectedSim3.find(pKF);
    if (it != NonCorrectedSim3.end()) put(it->second, &Snc[8 * (size_t)k]);
    else std::memcpy(&Snc[8 * (size_t)k], &Scw[8 * (size_t)k], 64);
  }
  // :975-1138: the edges.  An edge that would touch a keyframe without a vertex is not added.
  const int minFeat = 100;
  std::vector<int32_t> v0, v1;
  std::vector<uint8_t> kind;
  const auto add = [&](KeyFrame* i, KeyFrame* j, int k) {
    if (!index.count(i) || !index.count(j)) return;
    v0.push_back(index[i]);
    v1.push_back(index[j]);
    kind.push_back((uint8_t)k);
  };
  std::set<std::pair<long unsigned int, long unsigned int>> sInsertedEdges;
  std::vector<KeyFrame*> vLoopKeys;
  for (const auto& kv : LoopConnections) vLoopKeys.push_back(kv.first);
  std::sort(vLoopKeys.begin(), vLoopKeys.end(), byId);
  for (KeyFrame* pKF : vLoopKeys) {  // Set Loop edges (:981-1019)
    const long unsigned int nIDi = pKF->mnId;
    const std::set<KeyFrame*>& spConnections = LoopConnections.at(pKF);
    std::vector<KeyFrame*> vConn(spConnections.begin(), spConnections.end());
    std::sort(vConn.begin(), vConn.end(), byId);
    for (KeyFrame* pKFj : vConn) {
      const long unsigned int nIDj = pKFj->mnId;
      if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(pKFj) < minFeat) continue;
      add(pKF, pKFj, 0);
      sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
    }
  }
  for (KeyFrame* pKF : vertices) {  // Set normal edges (:1024-1138)
    KeyFrame* pParentKF = pKF->GetParent();
    if (pParentKF) add(pKF, pParentKF, 1);  // spanning tree edge
    const std::set<KeyFrame*> sLoopEdges = pKF->GetLoopEdges();
    std::vector<KeyFrame*> vLoopEdges(sLoopEdges.begin(), sLoopEdges.end());
    std::sort(vLoopEdges.begin(), vLoopEdges.end(), byId);
    for (KeyFrame* pLKF : vLoopEdges)
      if (pLKF->mnId < pKF->mnId) add(pKF, pLKF, 1);
    const std::vector<KeyFrame*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
    for (KeyFrame* pKFn : vpConnectedKFs) {
      if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
        if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
          if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId))))
            continue;
          add(pKF, pKFn, 1);
        }
      }
    }
  }
  // :1177-1196: the points that are not bad, each with the vertex of nIDr
  std::map<long unsigned int, int> indexOfId;
  for (int k = 0; k < n; k++) indexOfId[vertices[k]->mnId] = k;
  std::vector<MapPoint*> moved;
  std::vector<float> Xw;
  std::vector<int32_t> ref;
  for (MapPoint* pMP : vpMPs) {
    if (pMP->isBad()) continue;
    long unsigned int nIDr;
    if (pMP->mnCorrectedByKF == pCurKF->mnId) {
      nIDr = pMP->mnCorrectedReference;
    } else {
      KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
      nIDr = pRefKF->mnId;
    }
    const auto it = indexOfId.find(nIDr);
    if (it == indexOfId.end()) continue;
    const cv::Mat P3Dw = pMP->GetWorldPos();
    for (int k = 0; k < 3; k++) Xw.push_back(P3Dw.at<float>(k, 0));
    ref.push_back(it->second);
    moved.push_back(pMP);
  }
  orbx_essential_graph_problem p;
  std::memset(&p, 0, sizeof(p));
  p.n_vertices = n;
  p.vertex_id = ids.data();
  p.Scw = Scw.data();
  p.Snc = Snc.data();
  p.fixed_vertex = index.count(pLoopKF) ? index[pLoopKF] : -1;
  p.fix_scale = bFixScale ? 1 : 0;
  p.n_edges = (int)v0.size();
  p.edge_v0 = v0.data();
  p.edge_v1 = v1.data();
  p.edge_kind = kind.data();
  p.iterations = 20;
  p.lambda_init = 1e-16;
  p.n_points = (int)moved.size();
  p.Xw = Xw.data();
  p.point_ref = ref.data();
  std::vector<double> So(8 * (size_t)n);
  std::vector<float> To(12 * (size_t)n), Xo(3 * moved.size() + 3);
  orbx_essential_graph_result r;
  std::memset(&r, 0, sizeof(r));
  r.Scw_out = So.data();
  r.Tcw_out = To.data();
  r.Xw_out = Xo.data();
  check(orbx_optimize_essential_graph(&p, &r, gOrbxDevice), "orbx_optimize_essential_graph");
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  for (int k = 0; k < n; k++) {  // :1148-1172: SE3 pose recovering, [R t/s; 0 1]
    cv::Mat Tiw(4, 4, CV_32F);
    for (int i = 0; i < 12; i++) Tiw.at<float>(i / 4, i % 4) = To[12 * (size_t)k + i];
    for (int c = 0; c < 4; c++) Tiw.at<float>(3, c) = c == 3 ? 1.f : 0.f;
    vertices[k]->SetPose(Tiw);
  }
  for (size_t j = 0; j < moved.size(); j++) {  // :1177-1217: correct points
    cv::Mat cvCorrectedP3Dw(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) cvCorrectedP3Dw.at<float>(k, 0) = Xo[3 * j + k];
    moved[j]->SetWorldPos(cvCorrectedP3Dw);
    moved[j]->UpdateNormalAndDepth();
  }
}

void Optimizer::GlobalBundleAdjustemnt(Map* pMap, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF,
                                       const bool bRobust) {
  std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
  std::vector<MapPoint*> vpMP = pMap->GetAllMapPoints();
  BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust);
}

void Optimizer::BundleAdjustment(const std::vector<KeyFrame*>& vpKFsIn, const std::vector<MapPoint*>& vpMPIn,
                                 int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust) {
  // ascending mnId, as OptimizeEssentialGraph walks its containers (the caller's vectors come out of
  // pointer-ordered sets)
  std::vector<KeyFrame*> vpKFs(vpKFsIn);
  std::vector<MapPoint*> vpMP(vpMPIn);
  std::stable_sort(vpKFs.begin(), vpKFs.end(), [](KeyFrame* a, KeyFrame* b) { return a->mnId < b->mnId; });
  std::stable_sort(vpMP.begin(), vpMP.end(), [](MapPoint* a, MapPoint* b) { return a->mnId < b->mnId; });
  // src/Optimizer.cc:75-93: a vertex per keyframe that is not bad, fixed for mnId == 0
  std::vector<KeyFrame*> cams;
  std::map<KeyFrame*, int> cam_index;
  std::vector<float> Tcw, intr;
  std::vector<uint8_t> fixed;
  long unsigned int maxKFid = 0;
  for (KeyFrame* pKF : vpKFs) {
    if (pKF->isBad()) continue;
    cam_index[pKF] = (int)cams.size();
    cams.push_back(pKF);
    const cv::Mat T = pKF->GetPose();
    for (int i = 0; i < 12; i++) Tcw.push_back(T.at<float>(i / 4, i % 4));
    fixed.push_back(pKF->mnId == 0 ? 1 : 0);
    const float in[5] = {pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mbf};
    intr.insert(intr.end(), in, in + 5);
    if (pKF->mnId > maxKFid) maxKFid = pKF->mnId;
  }
  // :102-218: a vertex per point that is not bad, an edge per observation by a keyframe that is not bad
  // and not newer than maxKFid (monocular when mvuRight < 0)
  std::vector<MapPoint*> points;
  std::vector<float> Xw, obs, isig;
  std::vector<int32_t> ep, ec;
  for (MapPoint* pMP : vpMP) {
    if (pMP->isBad()) continue;
    const int p = (int)points.size();
    points.push_back(pMP);
    const cv::Mat X = pMP->GetWorldPos();
    for (int k = 0; k < 3; k++) Xw.push_back(X.at<float>(k, 0));
    const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
    std::vector<std::pair<KeyFrame*, size_t>> vObs(observations.begin(), observations.end());
    std::stable_sort(vObs.begin(), vObs.end(),
                     [](const std::pair<KeyFrame*, size_t>& a, const std::pair<KeyFrame*, size_t>& b) {
                       return a.first->mnId < b.first->mnId;
                     });
    for (const auto& ob : vObs) {
      KeyFrame* pKF = ob.first;
      if (pKF->isBad() || pKF->mnId > maxKFid) continue;
      const auto it = cam_index.find(pKF);
      if (it == cam_index.end()) continue;  // no vertex: g2o refuses the edge
      const cv::KeyPoint& kpUn = pKF->mvKeysUn[ob.second];
      ep.push_back(p);
      ec.push_back(it->second);
      obs.push_back(kpUn.pt.x);
      obs.push_back(kpUn.pt.y);
      obs.push_back(pKF->mvuRight[ob.second]);
      isig.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
    }
  }
  const int nc = (int)cams.size(), np = (int)points.size(), ne = (int)ep.size();
  orbx_ba_problem prob{nc, Tcw.data(), fixed.data(), intr.data(), np, Xw.data(),
                       ne, ep.data(), ec.data(), obs.data(), isig.data()};
  std::vector<float> Tout(12 * (size_t)nc + 1), Xout(3 * (size_t)np + 1);
  std::vector<uint8_t> included((size_t)np + 1);
  orbx_ba_result res;
  std::memset(&res, 0, sizeof(res));
  res.Tcw = Tout.data();
  res.Xw = Xout.data();
  // the calling thread keeps one solver (LoopClosing's GBA thread, or Tracking's for the monocular
  // bootstrap), released when that thread exits
  struct BaDeleter {
    void operator()(orbx_ba* h) const { orbx_ba_destroy(h); }
  };
  static thread_local std::unique_ptr<orbx_ba, BaDeleter> ba;
  static thread_local int ba_device = -1;
  if (ba && ba_device != gOrbxDevice) ba.reset();
  if (!ba) {
    orbx_ba* h = nullptr;
    check(orbx_ba_create(gOrbxDevice, &h), "orbx_ba_create");
    ba.reset(h);
    ba_device = gOrbxDevice;
  }
  check(orbx_ba_run_global_bool(ba.get(), &prob, nIterations, bRobust ? 1 : 0, &res, included.data(), pbStopFlag),
        "orbx_ba_run_global");
  // :228-251 keyframes
  for (int c = 0; c < nc; c++) {
    cv::Mat T(4, 4, CV_32F);
    for (int i = 0; i < 12; i++) T.at<float>(i / 4, i % 4) = Tout[12 * (size_t)c + i];
    for (int k = 0; k < 4; k++) T.at<float>(3, k) = k == 3 ? 1.f : 0.f;
    if (nLoopKF == 0) {
      cams[c]->SetPose(T);
    } else {
      cams[c]->mTcwGBA.create(4, 4, CV_32F);
      T.copyTo(cams[c]->mTcwGBA);
      cams[c]->mnBAGlobalForKF = nLoopKF;
    }
  }
  // :253-282 points (vbNotIncludedMP: a point that ended with no edge is skipped)
  for (int p = 0; p < np; p++) {
    if (!included[p]) continue;
    cv::Mat X(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) X.at<float>(k, 0) = Xout[3 * (size_t)p + k];
    if (nLoopKF == 0) {
      points[p]->SetWorldPos(X);
      points[p]->UpdateNormalAndDepth();
    } else {
      points[p]->mPosGBA.create(3, 1, CV_32F);
      X.copyTo(points[p]->mPosGBA);
      points[p]->mnBAGlobalForKF = nLoopKF;
    }
  }
}

void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap) {
  // src/Optimizer.cc:532-551: the local KeyFrames (pKF and its non-bad covisibles)
  std::list<KeyFrame*> lLocalKeyFrames;
  lLocalKeyFrames.push_back(pKF);
  pKF->mnBALocalForKF = pKF->mnId;
  const std::vector<KeyFrame*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
  for (KeyFrame* pKFi : vNeighKFs) {
    pKFi->mnBALocalForKF = pKF->mnId;
    if (!pKFi->isBad()) lLocalKeyFrames.push_back(pKFi);
  }
  // :553-572: the local MapPoints, first seen first
  std::list<MapPoint*> lLocalMapPoints;
  for (KeyFrame* pKFl : lLocalKeyFrames) {
    const std::vector<MapPoint*> vpMPs = pKFl->GetMapPointMatches();
    for (MapPoint* pMP : vpMPs)
      if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pKF->mnId) {
        lLocalMapPoints.push_back(pMP);
        pMP->mnBALocalForKF = pKF->mnId;
      }
  }
  // :574-592: KeyFrames that observe local MapPoints but are not local -> fixed
  std::list<KeyFrame*> lFixedCameras;
  for (MapPoint* pMP : lLocalMapPoints) {
    const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
    for (const auto& ob : observations) {
      KeyFrame* pKFi = ob.first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
        pKFi->mnBAFixedForKF = pKF->mnId;
        if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
      }
    }
  }
  // :608-640: vertices -- local poses (fixed iff mnId == 0), then the fixed cameras
  LocalBAProblem P;
  std::vector<KeyFrame*> cams;
  std::map<KeyFrame*, int> cam_index;
  auto add_cam = [&](KeyFrame* pKFi, bool fixed) {
    cam_index[pKFi] = (int)cams.size();
    cams.push_back(pKFi);
    LocalBAProblem::Camera C;
    C.Tcw = pKFi->GetPose();
    C.fixed = fixed;
    C.fx = pKFi->fx;
    C.fy = pKFi->fy;
    C.cx = pKFi->cx;
    C.cy = pKFi->cy;
    C.bf = pKFi->mbf;
    P.cameras.push_back(C);
  };
  for (KeyFrame* pKFi : lLocalKeyFrames) add_cam(pKFi, pKFi->mnId == 0);
  for (KeyFrame* pKFi : lFixedCameras) add_cam(pKFi, true);
  // :656-745: one point vertex per local MapPoint, one edge per observation by a non-bad KeyFrame
  // (GetObservations() order), monocular when mvuRight < 0
  std::vector<MapPoint*> points(lLocalMapPoints.begin(), lLocalMapPoints.end());
  std::vector<std::pair<KeyFrame*, MapPoint*>> edge_obj;
  for (size_t p = 0; p < points.size(); p++) {
    MapPoint* pMP = points[p];
    P.points.push_back(pMP->GetWorldPos());
    const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
    for (const auto& ob : observations) {
      KeyFrame* pKFi = ob.first;
      if (pKFi->isBad()) continue;
      const cv::KeyPoint& kpUn = pKFi->mvKeysUn[ob.second];
      LocalBAProblem::Observation o;
      o.point = (int)p;
      o.camera = cam_index.at(pKFi);
      o.u = kpUn.pt.x;
      o.v = kpUn.pt.y;
      o.ur = pKFi->mvuRight[ob.second];
      o.invSigma2 = pKFi->mvInvLevelSigma2[kpUn.octave];
      P.observations.push_back(o);
      edge_obj.emplace_back(pKFi, pMP);
    }
  }
  if (mpfnGatheredHook) mpfnGatheredHook(P, cams);
  // :747-751: a stop requested before the optimisation leaves the map untouched
  if (pbStopFlag && *pbStopFlag) return;
  LocalBAResult R;
  LocalBundleAdjustment(P, pbStopFlag, R, gOrbxDevice);
  // the flag may have gone up between the check above and the library's own poll: the library then
  // skipped optimize(5), and the reference would have returned here with the map untouched (:749-751)
  if (!R.ran) return;
  // :803-847 vToErase (the library's per-edge verdict after the last phase), then :849-884
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  for (size_t e = 0; e < edge_obj.size(); e++) {
    if (!R.erase[e]) continue;
    KeyFrame* pKFi = edge_obj[e].first;
    MapPoint* pMPi = edge_obj[e].second;
    pKFi->EraseMapPointMatch(pMPi);
    pMPi->EraseObservation(pKFi);
  }
  for (KeyFrame* pKFl : lLocalKeyFrames) pKFl->SetPose(R.Tcw[cam_index.at(pKFl)]);
  for (size_t p = 0; p < points.size(); p++) {
    points[p]->SetWorldPos(R.points[p]);
    points[p]->UpdateNormalAndDepth();
  }
}

void Optimizer::LocalBundleAdjustment(const LocalBAProblem& P, bool* pbStopFlag, LocalBAResult& R, int device) {
  const int nc = (int)P.cameras.size(), np = (int)P.points.size(), ne = (int)P.observations.size();
  std::vector<float> Tcw(12 * (size_t)nc), intr(5 * (size_t)nc), Xw(3 * (size_t)np), obs(3 * (size_t)ne),
      isig(ne);
  std::vector<uint8_t> fixed(nc);
  std::vector<int32_t> ep(ne), ec(ne);
  for (int c = 0; c < nc; c++) {
    const LocalBAProblem::Camera& C = P.cameras[c];
    for (int r = 0; r < 3; r++)
      for (int k = 0; k < 4; k++) Tcw[12 * c + 4 * r + k] = C.Tcw.at<float>(r, k);
    fixed[c] = C.fixed;
    const float in[5] = {C.fx, C.fy, C.cx, C.cy, C.bf};
    std::memcpy(&intr[5 * c], in, sizeof(in));
  }
  for (int p = 0; p < np; p++)
    for (int k = 0; k < 3; k++) Xw[3 * p + k] = P.points[p].at<float>(k, 0);
  for (int e = 0; e < ne; e++) {
    const LocalBAProblem::Observation& o = P.observations[e];
    ep[e] = o.point;
    ec[e] = o.camera;
    obs[3 * e] = o.u;
    obs[3 * e + 1] = o.v;
    obs[3 * e + 2] = o.ur;
    isig[e] = o.invSigma2;
  }
  orbx_ba_problem prob{nc, Tcw.data(), fixed.data(), intr.data(), np, Xw.data(),
                       ne, ep.data(), ec.data(), obs.data(), isig.data()};
  std::vector<float> Tout(12 * (size_t)nc), Xout(3 * (size_t)np);
  std::vector<uint8_t> erase(ne > 0 ? ne : 1);
  orbx_ba_result res;
  std::memset(&res, 0, sizeof(res));
  res.Tcw = Tout.data();
  res.Xw = Xout.data();
  res.edge_outlier = erase.data();
  // the LocalMapping thread keeps one solver (device buffers and stream reused across calls),
  // released when that thread exits
  struct BaDeleter {
    void operator()(orbx_ba* h) const { orbx_ba_destroy(h); }
  };
  static thread_local std::unique_ptr<orbx_ba, BaDeleter> ba;
  static thread_local int ba_device = -1;
  if (ba && ba_device != device) ba.reset();
  if (!ba) {
    orbx_ba* h = nullptr;
    check(orbx_ba_create(device, &h), "orbx_ba_create");
    ba.reset(h);
    ba_device = device;
  }
  check(orbx_ba_run_bool(ba.get(), &prob, &res, pbStopFlag), "orbx_ba_run");
  R.Tcw.resize(nc);
  for (int c = 0; c < nc; c++) {
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 3; r++)
      for (int k = 0; k < 4; k++) T.at<float>(r, k) = Tout[12 * c + 4 * r + k];
    T.at<float>(3, 0) = T.at<float>(3, 1) = T.at<float>(3, 2) = 0.f;
    T.at<float>(3, 3) = 1.f;
    R.Tcw[c] = T;
  }
  R.points.resize(np);
  for (int p = 0; p < np; p++) {
    cv::Mat X(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) X.at<float>(k, 0) = Xout[3 * p + k];
    R.points[p] = X;
  }
  R.erase.assign(ne, false);
  for (int e = 0; e < ne; e++) R.erase[e] = erase[e] != 0;
  R.iterations[0] = res.iterations[0];
  R.iterations[1] = res.iterations[1];
  R.trials = res.trials;
  R.ran = res.ran != 0;
}

}  // namespace ORB_SLAM2
