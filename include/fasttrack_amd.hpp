// fasttrack_amd.hpp - header-only C++ mirror of the reference's operator interface for the hot path,
// on top of the C ABI (fasttrack_amd.h).  Same names, argument meaning and return conventions as
//   ORB_SLAM3::ORBextractor           (reference include/ORBextractor.h:100-197)
//   KernelController::launch*         (reference include/Kernels/KernelController.h:13-55)
// but free of OpenCV / Eigen: images are (pointer, width, height, stride), keypoints are any struct
// with cv::KeyPoint's 28-byte layout (ft_keypoint, or cv::KeyPoint itself in an ORB-SLAM3 build), and
// descriptors are row-major N x 32 bytes (what a CV_8U cv::Mat holds).  INTEGRATION.md shows the
// few lines that bind it to cv::Mat / ORB_SLAM3::Frame.
//
// Errors: the reference prints and exit()s (src/Kernels/CudaUtils.cu:17-22); here every failure throws
// fasttrack::Error carrying ft_last_error().  There is no CPU run mode to fall back to: the five
// setGPURunMode flags of the reference have no equivalent.
#pragma once

#include <algorithm>
#include <array>
#include <cstring>
#include <functional>
#include <map>
#include <stdexcept>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "fasttrack_amd.h"

namespace fasttrack {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string &m) : std::runtime_error("fasttrack_amd: " + m), status(s) {}
};
inline void check(int status) {
    if (status != FT_OK) throw Error(status, ft_last_error());
}

// KernelController::setCUDADevice + initializeKernels + shutdownKernels + saveKernelsStats
class Context {
public:
    explicit Context(int device = 0, int hostThreads = 0) { check(ft_context_create(device, hostThreads, &h_)); }
    // ft_context_destroy refuses while extractors, front ends or tracked frames of the context are alive (they hold its
    // streams): a destructor cannot throw, so that ordering mistake is reported on stderr instead of leaking silently.
    // Declare the Context BEFORE the objects that use it (members are destroyed in reverse order).
    ~Context() {
        if (h_ && ft_context_destroy(h_) != FT_OK)
            std::fprintf(stderr, "fasttrack_amd: context not destroyed (leaked): %s\n", ft_last_error());
    }
    void setOption(const char *name, int value) { check(ft_context_set_option(h_, name, value)); }
    int getOption(const char *name) const {
        int v = 0;
        check(ft_context_get_option(h_, name, &v));
        return v;
    }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    ft_context *handle() const { return h_; }
    void synchronize() { check(ft_context_synchronize(h_)); }
    void saveKernelsStats(const std::string &file_path) { check(ft_context_save_stats(h_, file_path.c_str())); }

private:
    ft_context *h_ = nullptr;
};

// Non-owning 8-bit single-channel image (cv::Mat of type CV_8UC1: data, cols, rows, step[0]).
struct ImageView {
    const uint8_t *data = nullptr;
    int cols = 0, rows = 0, step = 0;
    bool empty() const { return !data || cols <= 0 || rows <= 0; }
};

template <class KeyPointT = ft_keypoint>
class ORBextractor {
    static_assert(sizeof(KeyPointT) == sizeof(ft_keypoint), "KeyPointT must have cv::KeyPoint's 28-byte layout");

public:
    // ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int imageWidth, int imageHeight)
    ORBextractor(Context &ctx, int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                 int imageWidth, int imageHeight, int maxBatch = 1)
        : nfeatures(nfeatures), scaleFactor(scaleFactor), nlevels(nlevels), iniThFAST(iniThFAST), minThFAST(minThFAST) {
        check(ft_extractor_create(ctx.handle(), nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, imageWidth,
                                  imageHeight, maxBatch, &h_));
        mvScaleFactor.resize(nlevels);
        mvInvScaleFactor.resize(nlevels);
        mvLevelSigma2.resize(nlevels);
        mvInvLevelSigma2.resize(nlevels);
        check(ft_extractor_scale_factors(h_, mvScaleFactor.data(), mvInvScaleFactor.data(), mvLevelSigma2.data(),
                                         mvInvLevelSigma2.data()));
    }
    ~ORBextractor() { ft_extractor_destroy(h_); }
    ORBextractor(const ORBextractor &) = delete;
    ORBextractor &operator=(const ORBextractor &) = delete;

    // int operator()(InputArray image, InputArray mask, vector<KeyPoint>& keypoints, OutputArray descriptors,
    //                std::vector<int>& vLappingArea)        (the mask is ignored by the reference too)
    // descriptors: resized to keypoints.size() * 32 bytes (rows of a CV_8U N x 32 matrix).
    // Returns the reference's monoIndex, or -1 for an empty image (ORBextractor.cc:1360-1361).
    int operator()(const ImageView &image, std::vector<KeyPointT> &keypoints, std::vector<uint8_t> &descriptors,
                   const std::vector<int> &vLappingArea) {
        if (image.empty()) return -1;
        const int cap = ft_extractor_max_keypoints(h_);
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0, nMono = 0;
        const int lap0 = vLappingArea.size() > 0 ? vLappingArea[0] : 0, lap1 = vLappingArea.size() > 1 ? vLappingArea[1] : 0;
        const int st = ft_extract(h_, image.data, image.cols, image.rows, image.step, lap0, lap1,
                                  reinterpret_cast<ft_keypoint *>(keypoints.data()), descriptors.data(), cap, &n, &nMono);
        if (st == FT_ERR_EMPTY) return -1;
        check(st);
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);
        return nMono;
    }

    int inline GetLevels() { return nlevels; }
    float inline GetScaleFactor() { return scaleFactor; }
    std::vector<float> inline GetScaleFactors() { return mvScaleFactor; }
    std::vector<float> inline GetInverseScaleFactors() { return mvInvScaleFactor; }
    std::vector<float> inline GetScaleSigmaSquares() { return mvLevelSigma2; }
    std::vector<float> inline GetInverseScaleSigmaSquares() { return mvInvLevelSigma2; }

    // mvImagePyramid[level]: host copy of one level of the last image (the reference keeps bordered
    // cv::Mat ROIs; nothing on the path reads the border, so tight rows are returned)
    std::vector<uint8_t> imagePyramidLevel(int level, int &cols, int &rows, int slot = 0) {
        check(ft_extractor_level_size(h_, level, &cols, &rows));
        std::vector<uint8_t> out((size_t)cols * rows);
        check(ft_extractor_download_level(h_, slot, level, out.data(), cols));
        return out;
    }
    // GetGPUPyramid(): device pointer + pitch of a level
    const uint8_t *GetGPUPyramid(int level, int &pitch, int slot = 0) {
        const uint8_t *p = nullptr;
        check(ft_extractor_device_level(h_, slot, level, &p, &pitch));
        return p;
    }
    ft_extractor *handle() const { return h_; }

    const int nfeatures;
    const float scaleFactor;
    const int nlevels, iniThFAST, minThFAST;

private:
    ft_extractor *h_ = nullptr;
    std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
};

// Static facade with the reference's launch* names.  Outputs follow the reference's own conventions:
// vectors are resized by the callee, int arrays are caller-allocated.
struct KernelController {
    // launchStereoMatchKernel(vRowIndices, d_pyrL, d_pyrR, pyrL, pyrR, keysL, keysR, descL, descR, minD, maxD,
    //                         thOrbDist, mbf, pyramidOnGpu, vDistIdx, mvuRight, mvDepth)     KernelController.h:31-36
    // The row table and the pyramids live on the device already (slot `slot` of both extractors), minD/maxD
    // follow from mb/mbf as in Frame.cc:864-867.  vDistIdx receives (SAD, iL) of every refined match so the
    // caller's median cut (Frame.cc:1049-1062) runs unchanged when applyMedianCut is false.
    template <class KP>
    static void launchStereoMatchKernel(ORBextractor<KP> &left, ORBextractor<KP> &right, const std::vector<KP> &mvKeys,
                                        const std::vector<KP> &mvKeysRight, const uint8_t *mDescriptors,
                                        const uint8_t *mDescriptorsRight, float mbf, float mb, bool applyMedianCut,
                                        std::vector<std::pair<int, int>> &vDistIdx, std::vector<float> &mvuRight,
                                        std::vector<float> &mvDepth, int slot = 0) {
        const int N = (int)mvKeys.size(), Nr = (int)mvKeysRight.size();
        mvuRight.assign(N, -1.0f);
        mvDepth.assign(N, -1.0f);
        std::vector<int> sad(N > 0 ? N : 1, -1);
        int nm = 0;
        check(ft_stereo_match(left.handle(), right.handle(), slot, reinterpret_cast<const ft_keypoint *>(mvKeys.data()), N,
                              reinterpret_cast<const ft_keypoint *>(mvKeysRight.data()), Nr, mDescriptors,
                              mDescriptorsRight, mbf, mb, applyMedianCut ? 1 : 0, mvuRight.data(), mvDepth.data(),
                              sad.data(), &nm));
        vDistIdx.clear();
        for (int i = 0; i < N; i++)
            if (sad[i] >= 0) vDistIdx.push_back(std::make_pair(sad[i], i));
    }

    // launchFisheyeStereoMatchKernel(N, Nr, descL, descR, matches)                         KernelController.h:38
    static void launchFisheyeStereoMatchKernel(Context &ctx, int N, int Nr, const uint8_t *mDescriptors,
                                               const uint8_t *mDescriptorsRight, int *matches) {
        check(ft_fisheye_match(ctx.handle(), mDescriptors, N, mDescriptorsRight, Nr, matches, nullptr, nullptr));
    }

    // Frame::ComputeStereoFishEyeMatches complete (src/Frame.cc:1231-1271): ratio-tested 2-NN matches filtered by
    // KannalaBrandt8::TriangulateMatches.  Arrays are indexed like the lapping-area subsets.
    static int computeStereoFishEyeMatches(Context &ctx, const ft_fisheye_rig &rig, int N, int Nr, const uint8_t *descL,
                                           const ft_keypoint *keysL, const uint8_t *descR, const ft_keypoint *keysR,
                                           const std::vector<float> &mvLevelSigma2, std::vector<int> &leftToRight,
                                           std::vector<float> &mvDepth, std::vector<float> &mvStereo3Dpoints) {
        leftToRight.assign(N > 0 ? N : 1, -1);
        mvDepth.assign(N > 0 ? N : 1, -1.0f);
        mvStereo3Dpoints.assign(3 * (size_t)(N > 0 ? N : 1), 0.f);
        int nm = 0;
        check(ft_fisheye_stereo(ctx.handle(), &rig, descL, keysL, N, descR, keysR, Nr, mvLevelSigma2.data(),
                                (int)mvLevelSigma2.size(), leftToRight.data(), mvDepth.data(), mvStereo3Dpoints.data(), &nm));
        leftToRight.resize(N);
        mvDepth.resize(N);
        mvStereo3Dpoints.resize(3 * (size_t)N);
        return nm;
    }

    // launchSearchLocalPointsKernel(F, vmp, th, bFarPoints, thFarPoints, 10 x int*)        KernelController.h:40-42
    // F / P are the POD views of Frame and of the map points (INTEGRATION.md shows how they are filled);
    // in addition to the ten raw arrays the call returns the final assignment and nmatches, i.e. the
    // acceptance loop of ORBmatcher.cc:241-308 is included.
    static int launchSearchLocalPointsKernel(Context &ctx, ft_frame_view &F, const ft_local_points &P, float th,
                                             float mfNNratio, std::vector<int> &assign, int *h_bestLevel,
                                             int *h_bestLevel2, int *h_bestDist, int *h_bestDist2, int *h_bestIdx,
                                             int *h_bestLevelR, int *h_bestLevelR2, int *h_bestDistR, int *h_bestDistR2,
                                             int *h_bestIdxR) {
        assign.assign(F.N > 0 ? F.N : 1, -1);
        int nm = 0;
        check(ft_search_local_points(ctx.handle(), &F, &P, th, mfNNratio, assign.data(), &nm, h_bestDist, h_bestDist2,
                                     h_bestLevel, h_bestLevel2, h_bestIdx, h_bestDistR, h_bestDistR2,
                                     h_bestLevelR, h_bestLevelR2, h_bestIdxR));
        assign.resize(F.N);
        return nm;
    }

    // launchPoseEstimationKernel(Cur, Last, th, bForward, bBackward, Tcw, 4 x int*)        KernelController.h:44-46
    // Tcw: row-major 3x4 (the top rows of the reference's Eigen::Matrix4f).
    static int launchPoseEstimationKernel(Context &ctx, ft_frame_view &CurrentFrame, const ft_last_points &LastFrame,
                                          float th, bool bForward, bool bBackward, const float *Tcw,
                                          bool mbCheckOrientation, std::vector<int> &assign, int *h_bestDist,
                                          int *h_bestIdx2, int *h_bestDistR, int *h_bestIdxR2) {
        assign.assign(CurrentFrame.N > 0 ? CurrentFrame.N : 1, -1);
        int nm = 0;
        check(ft_search_last_frame(ctx.handle(), &CurrentFrame, &LastFrame, Tcw, th, bForward ? 1 : 0, bBackward ? 1 : 0,
                                   mbCheckOrientation ? 1 : 0, assign.data(), &nm, h_bestDist, h_bestIdx2, h_bestDistR,
                                   h_bestIdxR2));
        assign.resize(CurrentFrame.N);
        return nm;
    }
    // The same with the poses as the CPU branch multiplies with them (Sophus::SE3f: `Tcw * x3Dw`, ORBmatcher.cc:1805, is a
    // quaternion rotation): Tcw = se3Of(CurrentFrame.GetPose()), Trl = se3Of(CurrentFrame.GetRelativePoseTrl()) or nullptr for
    // one camera.  Bit-for-bit the CPU branch; the matrix overload above is the reference's GPU boundary.
    static int launchPoseEstimationKernel(Context &ctx, ft_frame_view &CurrentFrame, const ft_last_points &LastFrame,
                                          float th, bool bForward, bool bBackward, const ft_se3 &Tcw, const ft_se3 *Trl,
                                          bool mbCheckOrientation, std::vector<int> &assign, int *h_bestDist,
                                          int *h_bestIdx2, int *h_bestDistR, int *h_bestIdxR2) {
        assign.assign(CurrentFrame.N > 0 ? CurrentFrame.N : 1, -1);
        int nm = 0;
        check(ft_search_last_frame_se3(ctx.handle(), &CurrentFrame, &LastFrame, &Tcw, Trl, th, bForward ? 1 : 0, bBackward ? 1 : 0,
                                       mbCheckOrientation ? 1 : 0, assign.data(), &nm, h_bestDist, h_bestIdx2, h_bestDistR,
                                       h_bestIdxR2));
        assign.resize(CurrentFrame.N);
        return nm;
    }
    // ORBmatcher(0.9, mbCheckOrientation).SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) on a frame view
    // (ORBmatcher.cc:2087-2208; the reference has no GPU boundary for it): pKF.valid carries sAlreadyFound, Tcw =
    // se3Of(CurrentFrame.GetPose()); h_bestDist / h_bestIdx2 (pKF.N ints, may be null): what the loop leaves per point
    static int SearchByProjection(Context &ctx, ft_frame_view &CurrentFrame, const ft_keyframe_points &pKF, const ft_se3 &Tcw,
                                  float mfLogScaleFactor, float th, int ORBdist, bool mbCheckOrientation, std::vector<int> &assign,
                                  int *h_bestDist = nullptr, int *h_bestIdx2 = nullptr) {
        assign.assign(CurrentFrame.N > 0 ? CurrentFrame.N : 1, -1);
        int nm = 0;
        check(ft_search_keyframe_projection(ctx.handle(), &CurrentFrame, &pKF, &Tcw, mfLogScaleFactor, th, ORBdist,
                                            mbCheckOrientation ? 1 : 0, assign.data(), &nm, h_bestDist, h_bestIdx2));
        assign.resize(CurrentFrame.N);
        return nm;
    }
};

// ft_se3 of a Sophus::SE3f (or anything with unit_quaternion().coeffs() = x y z w and translation()): the pose form of the
// CPU branch's point transforms
template <class SE3f>
inline ft_se3 se3Of(const SE3f &T) {
    ft_se3 r;
    const auto q = T.unit_quaternion().coeffs();
    const auto t = T.translation();
    for (int i = 0; i < 4; i++) r.q[i] = q[i];
    for (int i = 0; i < 3; i++) r.t[i] = t[i];
    return r;
}

// Frame::isInFrustum for all local map points (src/Frame.cc:536-610, 1308-1382; the loop of
// src/Tracking.cc:3503-3522).  The vectors receive the MapPoint tracking fields; returns nToMatch.
struct FrustumFields {
    std::vector<uint8_t> mbTrackInView, mbTrackInViewR;
    std::vector<int> mnTrackScaleLevel, mnTrackScaleLevelR;
    std::vector<float> mTrackViewCos, mTrackViewCosR, mTrackProjX, mTrackProjY, mTrackProjXR, mTrackProjYR, mTrackDepth,
        mTrackDepthR;
    ft_frustum_result view(int M) {
        const size_t m = M > 0 ? (size_t)M : 1;
        mbTrackInView.assign(m, 0); mbTrackInViewR.assign(m, 0);
        mnTrackScaleLevel.assign(m, -1); mnTrackScaleLevelR.assign(m, -1);
        for (auto *v : {&mTrackViewCos, &mTrackViewCosR, &mTrackProjX, &mTrackProjY, &mTrackProjXR, &mTrackProjYR, &mTrackDepth,
                        &mTrackDepthR})
            v->assign(m, 0.f);
        ft_frustum_result r;
        r.in_view = mbTrackInView.data(); r.in_view_r = mbTrackInViewR.data();
        r.level = mnTrackScaleLevel.data(); r.level_r = mnTrackScaleLevelR.data();
        r.view_cos = mTrackViewCos.data(); r.view_cos_r = mTrackViewCosR.data();
        r.proj_x = mTrackProjX.data(); r.proj_y = mTrackProjY.data();
        r.proj_xr = mTrackProjXR.data(); r.proj_yr = mTrackProjYR.data();
        r.depth = mTrackDepth.data(); r.depth_r = mTrackDepthR.data();
        return r;
    }
};

inline int isInFrustum(Context &ctx, const ft_frame_view &F, const ft_frame_pose &pose, const ft_map_points &P,
                       float viewingCosLimit, float mfLogScaleFactor, FrustumFields &out) {
    const ft_frustum_result r = out.view(P.M);
    int n = 0;
    check(ft_is_in_frustum(ctx.handle(), &F, &pose, &P, viewingCosLimit, mfLogScaleFactor, &r, &n));
    return n;
}

// Device-resident Frame for the projection searches (ft_tracked_frame_*): upload (or bind to a stereo front end
// slot) once per frame, then SearchByProjection(last frame) and SearchLocalPoints without re-marshalling.
class TrackedFrame {
public:
    TrackedFrame(Context &ctx, int maxKeypoints, int maxPoints) {
        check(ft_tracked_frame_create(ctx.handle(), maxKeypoints, maxPoints, &h_));
    }
    ~TrackedFrame() { ft_tracked_frame_destroy(h_); }
    TrackedFrame(const TrackedFrame &) = delete;
    TrackedFrame &operator=(const TrackedFrame &) = delete;
    void upload(const ft_frame_view &F) {
        check(ft_tracked_frame_upload(h_, &F));
        N_ = F.N;
    }
    void bindStereo(ft_stereo_frontend *fe, int slot, const ft_frame_view &meta) {
        check(ft_tracked_frame_bind_stereo(h_, fe, slot, &meta));
        N_ = meta.N;
    }
    // ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono)                       ORBmatcher.cc:1775
    int SearchByProjection(const ft_last_points &LastFrame, const float *Tcw, float th, bool bForward, bool bBackward,
                           bool mbCheckOrientation, std::vector<int> &assign) {
        assign.assign(N_ > 0 ? N_ : 1, -1);
        int nm = 0;
        check(ft_tracked_frame_search_last_frame(h_, &LastFrame, Tcw, th, bForward, bBackward, mbCheckOrientation,
                                                 assign.data(), &nm));
        assign.resize(N_);
        return nm;
    }
    int SearchByProjection(const ft_last_points &LastFrame, const ft_se3 &Tcw, const ft_se3 *Trl, float th, bool bForward,
                           bool bBackward, bool mbCheckOrientation, std::vector<int> &assign) {
        assign.assign(N_ > 0 ? N_ : 1, -1);
        int nm = 0;
        check(ft_tracked_frame_search_last_frame_se3(h_, &LastFrame, &Tcw, Trl, th, bForward, bBackward, mbCheckOrientation,
                                                     assign.data(), &nm));
        assign.resize(N_);
        return nm;
    }
    // ORBmatcher(0.9, mbCheckOrientation).SearchByProjection(CurrentFrame = *this, pKF, sAlreadyFound, th, ORBdist), the matcher of
    // Tracking::Relocalization                                                   ORBmatcher.cc:2087, Tracking.cc:3924, :3938
    // pKF: the keyframe's GetMapPointMatches() as arrays; sAlreadyFound is folded into pKF.valid (pMP && !pMP->isBad() &&
    // !sAlreadyFound.count(pMP)).  assign[i2] = the keyframe index whose point ends up in mvpMapPoints[i2], else -1.
    int SearchByProjection(const ft_keyframe_points &pKF, const ft_se3 &Tcw, float mfLogScaleFactor, float th, int ORBdist,
                           bool mbCheckOrientation, std::vector<int> &assign) {
        assign.assign(N_ > 0 ? N_ : 1, -1);
        int nm = 0;
        check(ft_tracked_frame_search_keyframe_projection(h_, &pKF, &Tcw, mfLogScaleFactor, th, ORBdist, mbCheckOrientation ? 1 : 0,
                                                          assign.data(), &nm));
        assign.resize(N_);
        return nm;
    }
    // Tracking::SearchLocalPoints: isInFrustum(pMP, 0.5) for every point + SearchByProjection(F, points, th, ...)
    int SearchLocalPoints(const ft_frame_pose &pose, const ft_map_points &P, float viewingCosLimit, float mfLogScaleFactor,
                          float th, float mfNNratio, bool bFarPoints, float thFarPoints, FrustumFields *fields,
                          int *nToMatch, std::vector<int> &assign) {
        assign.assign(N_ > 0 ? N_ : 1, -1);
        ft_frustum_result r;
        if (fields) r = fields->view(P.M);
        int nm = 0;
        check(ft_tracked_frame_track_local_map(h_, &pose, &P, viewingCosLimit, mfLogScaleFactor, th, mfNNratio, bFarPoints,
                                               thFarPoints, fields ? &r : nullptr, nToMatch, assign.data(), &nm));
        assign.resize(N_);
        return nm;
    }
    // ORBmatcher(mfNNratio, mbCheckOrientation).SearchForInitialization(F1, *this, vbPrevMatched, vnMatches12, windowSize)
    // with *this as the current frame F2 and F1 = mInitialFrame, both resident           ORBmatcher.cc:747, Tracking.cc:2516-2549
    // Point2f: cv::Point2f or anything else made of two floats x, y.
    template <class Point2f>
    int SearchForInitialization(TrackedFrame &F1, std::vector<Point2f> &vbPrevMatched, std::vector<int> &vnMatches12, int windowSize,
                                float mfNNratio = 0.9f, bool mbCheckOrientation = true) {
        static_assert(sizeof(Point2f) == 2 * sizeof(float), "vbPrevMatched must hold two floats per keypoint");
        if ((int)vbPrevMatched.size() != F1.N_) throw Error(FT_ERR_INVALID, "vbPrevMatched must hold one point per keypoint of F1");
        vnMatches12.assign(F1.N_ > 0 ? F1.N_ : 1, -1);
        int nm = 0;
        check(ft_tracked_frame_search_for_initialization(h_, F1.h_, reinterpret_cast<float *>(vbPrevMatched.data()), windowSize,
                                                         mfNNratio, mbCheckOrientation ? 1 : 0, vnMatches12.data(), &nm));
        vnMatches12.resize(F1.N_);
        return nm;
    }
    std::vector<int> holderObservations() {
        std::vector<int> h(N_ > 0 ? N_ : 1);
        check(ft_tracked_frame_holder_obs(h_, h.data()));
        h.resize(N_);
        return h;
    }
    ft_tracked_frame *handle() { return h_; }

private:
    ft_tracked_frame *h_ = nullptr;
    int N_ = 0;
};

// B frames per launch (ft_tracked_batch_*): the frames B camera streams deliver for one time step - or any B frames whose
// inputs the caller holds - searched through ONE set of launches; per frame the results of TrackedFrame's calls.  A batch has
// a stream of its own: several batches used from several host threads are several steps in flight.
class TrackedBatch {
public:
    TrackedBatch(Context &ctx, int maxFrames, int maxKeypoints, int maxPoints) {
        check(ft_tracked_batch_create(ctx.handle(), maxFrames, maxKeypoints, maxPoints, &h_));
    }
    ~TrackedBatch() { ft_tracked_batch_destroy(h_); }
    TrackedBatch(const TrackedBatch &) = delete;
    TrackedBatch &operator=(const TrackedBatch &) = delete;
    void upload(const std::vector<ft_frame_view> &frames) {
        check(ft_tracked_batch_upload(h_, (int)frames.size(), frames.data()));
        loaded(frames);
    }
    // the two-camera frames of the batch from what two extractors left in HBM (their last operator() batches): keypoints into
    // the reference's lapping-area order, the matching of Frame::ComputeStereoFishEyeMatches, the grids - all on the device
    // rig != nullptr: with KannalaBrandt8::TriangulateMatches on every matched pair (mvLevelSigma2 = levelSigma2), as
    // Frame::ComputeStereoFishEyeMatches; mvDepth / mvStereo3Dpoints / nMatches per frame on request
    void bindFisheye(ft_extractor *left, ft_extractor *right, int slot0, const int lapLeft[2], const int lapRight[2],
                     const std::vector<ft_frame_view> &meta, const ft_fisheye_rig *rig = nullptr, const float *levelSigma2 = nullptr,
                     int *const *leftToRight = nullptr, int *const *rightToLeft = nullptr, float *const *mvDepth = nullptr,
                     float *const *mvStereo3Dpoints = nullptr, int *nMatches = nullptr) {
        check(ft_tracked_batch_bind_fisheye(h_, left, right, slot0, (int)meta.size(), lapLeft[0], lapLeft[1], lapRight[0], lapRight[1],
                                            meta.data(), rig, levelSigma2, leftToRight, rightToLeft, mvDepth, mvStereo3Dpoints, nMatches));
        loaded(meta);
    }
    // ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for every frame; Tcw: 12 floats per frame     ORBmatcher.cc:1775
    void SearchByProjection(const std::vector<ft_last_points> &LastFrames, const float *Tcw, float th, bool mbCheckOrientation,
                            std::vector<std::vector<int>> &assign, std::vector<int> &nmatches, const int *bForward = nullptr,
                            const int *bBackward = nullptr) {
        prepare(assign, nmatches);
        check(ft_tracked_batch_search_last_frame(h_, (int)N_.size(), LastFrames.data(), Tcw, th, bForward, bBackward, mbCheckOrientation,
                                                 ptrs_.data(), nmatches.data()));
        finish(assign);
    }
    // Tracking::SearchLocalPoints for every frame: isInFrustum + SearchByProjection(F, points, th, ...)              Tracking.cc:3472
    void SearchLocalPoints(const std::vector<ft_frame_pose> &poses, const std::vector<ft_map_points> &P, float viewingCosLimit,
                           float mfLogScaleFactor, float th, float mfNNratio, bool bFarPoints, float thFarPoints,
                           const ft_frustum_result *fields, std::vector<int> &nToMatch, std::vector<std::vector<int>> &assign,
                           std::vector<int> &nmatches) {
        prepare(assign, nmatches);
        nToMatch.assign(N_.size(), 0);
        check(ft_tracked_batch_track_local_map(h_, (int)N_.size(), poses.data(), P.data(), viewingCosLimit, mfLogScaleFactor, th, mfNNratio,
                                               bFarPoints, thFarPoints, fields, nToMatch.data(), ptrs_.data(), nmatches.data()));
        finish(assign);
    }
    // The same two searches in two halves (ft_tracked_batch_submit_* / ft_tracked_batch_wait): submit enqueues and returns, Wait() fills
    // assign / nmatches (/ nToMatch) - they and the point arrays (when those lie in pinned memory) must stay as they are until then.
    void SubmitSearchByProjection(const std::vector<ft_last_points> &LastFrames, const float *Tcw, float th, bool mbCheckOrientation,
                                  std::vector<std::vector<int>> &assign, std::vector<int> &nmatches, const int *bForward = nullptr,
                                  const int *bBackward = nullptr) {
        prepare(assign, nmatches);
        pending_ = &assign;
        check(ft_tracked_batch_submit_search_last_frame(h_, (int)N_.size(), LastFrames.data(), Tcw, th, bForward, bBackward, mbCheckOrientation,
                                                        ptrs_.data(), nmatches.data()));
    }
    void SubmitSearchLocalPoints(const std::vector<ft_frame_pose> &poses, const std::vector<ft_map_points> &P, float viewingCosLimit,
                                 float mfLogScaleFactor, float th, float mfNNratio, bool bFarPoints, float thFarPoints,
                                 const ft_frustum_result *fields, std::vector<int> &nToMatch, std::vector<std::vector<int>> &assign,
                                 std::vector<int> &nmatches) {
        prepare(assign, nmatches);
        nToMatch.assign(N_.size(), 0);
        pending_ = &assign;
        check(ft_tracked_batch_submit_track_local_map(h_, (int)N_.size(), poses.data(), P.data(), viewingCosLimit, mfLogScaleFactor, th,
                                                      mfNNratio, bFarPoints, thFarPoints, fields, nToMatch.data(), ptrs_.data(), nmatches.data()));
    }
    void Wait() {
        check(ft_tracked_batch_wait(h_));
        if (pending_) finish(*pending_);
        pending_ = nullptr;
    }
    std::vector<int> holderObservations(int frame) {
        std::vector<int> h(N_[frame] > 0 ? N_[frame] : 1);
        check(ft_tracked_batch_holder_obs(h_, frame, h.data()));
        h.resize(N_[frame]);
        return h;
    }
    ft_tracked_batch *handle() { return h_; }

private:
    void loaded(const std::vector<ft_frame_view> &frames) {
        N_.clear();
        for (const ft_frame_view &F : frames) N_.push_back(F.N);
    }
    void prepare(std::vector<std::vector<int>> &assign, std::vector<int> &nmatches) {
        assign.resize(N_.size());
        ptrs_.resize(N_.size());
        nmatches.assign(N_.size(), 0);
        for (size_t f = 0; f < N_.size(); f++) {
            assign[f].assign(N_[f] > 0 ? N_[f] : 1, -1);
            ptrs_[f] = assign[f].data();
        }
    }
    void finish(std::vector<std::vector<int>> &assign) {
        for (size_t f = 0; f < N_.size(); f++) assign[f].resize(N_[f]);
    }
    ft_tracked_batch *h_ = nullptr;
    std::vector<int> N_;
    std::vector<int *> ptrs_;
    std::vector<std::vector<int>> *pending_ = nullptr;
};

// ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) for Frame::ComputeBoW: same call as
// mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4) (src/Frame.cc:762-769), with the tree walk on the
// device.  BowVector / FeatureVector are the std::map types of DBoW2 (BowVector.h:59, FeatureVector.h:24).
class ORBVocabulary {
public:
    typedef std::map<unsigned, double> BowVector;
    typedef std::map<unsigned, std::vector<unsigned>> FeatureVector;
    ORBVocabulary(Context &ctx, const std::string &textFile) { check(ft_vocabulary_load_text(ctx.handle(), textFile.c_str(), &h_)); }
    ~ORBVocabulary() { ft_vocabulary_destroy(h_); }
    ORBVocabulary(const ORBVocabulary &) = delete;
    ORBVocabulary &operator=(const ORBVocabulary &) = delete;
    // descriptors: N x 32 bytes (cv::Mat mDescriptors is continuous); onDevice: a pointer into HBM, e.g. from
    // ft_stereo_frontend_device_descriptors
    void transform(const uint8_t *descriptors, int N, BowVector &v, FeatureVector &fv, int levelsup, bool onDevice = false) {
        v.clear();
        fv.clear();
        if (N <= 0) return;
        std::vector<unsigned> ids(N), nodes(N), feats(N);
        std::vector<double> vals(N);
        std::vector<int> offs(N + 1);
        int nb = 0, nf = 0;
        check(ft_bow_transform(h_, descriptors, N, onDevice ? 1 : 0, levelsup, nullptr, nullptr, nullptr, ids.data(), vals.data(), N,
                               &nb, nodes.data(), offs.data(), feats.data(), N, &nf));
        for (int j = 0; j < nb; j++) v.emplace_hint(v.end(), ids[j], vals[j]);
        for (int j = 0; j < nf; j++)
            fv.emplace_hint(fv.end(), nodes[j], std::vector<unsigned>(feats.begin() + offs[j], feats.begin() + offs[j + 1]));
    }
    ft_vocabulary *handle() { return h_; }

private:
    ft_vocabulary *h_ = nullptr;
};

namespace detail {
// a std::map FeatureVector in the CSR form the C ABI takes, and the ft_bow_side over it
struct BowCsr {
    std::vector<unsigned> nodes, feats;
    std::vector<int> offs;
};
inline BowCsr flattenFeatVec(const ORBVocabulary::FeatureVector &fv) {
    BowCsr c;
    c.offs.push_back(0);
    for (const auto &e : fv) {
        c.nodes.push_back(e.first);
        c.feats.insert(c.feats.end(), e.second.begin(), e.second.end());
        c.offs.push_back((int)c.feats.size());
    }
    return c;
}
inline ft_bow_side bowSide(const BowCsr &c, int n, const uint8_t *d, const float *a) {
    ft_bow_side s;
    s.n = n;
    s.n_nodes = (int)c.nodes.size();
    s.fv_nodes = c.nodes.data();
    s.fv_offsets = c.offs.data();
    s.fv_features = c.feats.data();
    s.descriptors = d;
    s.angles = a;
    return s;
}
}  // namespace detail

// ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches) (src/ORBmatcher.cc:322-524) on the
// std::map FeatureVectors of ORBVocabulary::transform.  kfHasPoint[i] = vpMapPointsKF[i] && !vpMapPointsKF[i]->isBad();
// kfAngles / fAngles = cv::KeyPoint::angle per feature (right-camera features after the left ones, as the reference indexes
// them).  matches[i] = index into vpMapPointsKF or -1: `vpMapPointMatches[i] = matches[i] < 0 ? nullptr : vpMapPointsKF[matches[i]]`.
// Returns nmatches.
inline int SearchByBoW(Context &ctx, const ORBVocabulary::FeatureVector &kfFeatVec, const uint8_t *kfDescriptors, int kfN,
                       const std::vector<uint8_t> &kfHasPoint, const float *kfAngles, const ORBVocabulary::FeatureVector &fFeatVec,
                       const uint8_t *fDescriptors, int fN, const float *fAngles, int fNleft, float nnRatio, bool checkOrientation,
                       std::vector<int> &matches) {
    const detail::BowCsr k = detail::flattenFeatVec(kfFeatVec), f = detail::flattenFeatVec(fFeatVec);
    const ft_bow_side K = detail::bowSide(k, kfN, kfDescriptors, kfAngles), F = detail::bowSide(f, fN, fDescriptors, fAngles);
    matches.assign(fN > 0 ? fN : 1, -1);
    int nm = 0;
    check(ft_search_by_bow(ctx.handle(), &K, kfHasPoint.data(), &F, fNleft, nnRatio, checkOrientation ? 1 : 0, matches.data(), &nm));
    matches.resize(fN > 0 ? fN : 0);
    return nm;
}

// What ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vpMatches12) reads of a KeyFrame: mFeatVec, mDescriptors (N rows),
// hasPoint[i] = GetMapPoint(i) && !GetMapPoint(i)->isBad(), angles = cv::KeyPoint::angle of mvKeysUn (N entries; those from nUn on
// are not read), NLeft and nUn = mvKeysUn.size() (read only when NLeft != -1).
struct BowKeyFrame {
    const ORBVocabulary::FeatureVector *mFeatVec = nullptr;
    const uint8_t *mDescriptors = nullptr;
    int N = 0;
    const uint8_t *hasPoint = nullptr;
    const float *angles = nullptr;
    int NLeft = -1, nUn = 0;
};
// ORBmatcher(nnRatio, checkOrientation).SearchByBoW(pKF1, pKF2, vpMatches12) (src/ORBmatcher.cc:864-1004) for pKF1 against every
// keyframe of kf2s in one call (ft_search_by_bow_keyframes; LoopClosing::DetectCommonRegionsFromBoW, src/LoopClosing.cc:657-668).
// vvMatches12[k][idx1] = index into kf2s[k]'s GetMapPointMatches() or -1:
// `vpMatches12[idx1] = m < 0 ? nullptr : vpMapPoints2[m]`.  Returns nmatches per keyframe.
inline std::vector<int> SearchByBoW(Context &ctx, const BowKeyFrame &kf1, const std::vector<BowKeyFrame> &kf2s, float nnRatio,
                                    bool checkOrientation, std::vector<std::vector<int>> &vvMatches12) {
    const size_t nn = kf2s.size(), n1 = kf1.N > 0 ? (size_t)kf1.N : 0;
    std::vector<detail::BowCsr> csr(nn + 1);
    auto record = [&](const BowKeyFrame &k, detail::BowCsr &c) {
        if (!k.mFeatVec) throw std::invalid_argument("SearchByBoW: a keyframe without mFeatVec");
        c = detail::flattenFeatVec(*k.mFeatVec);
        ft_bow_keyframe r;
        r.side = detail::bowSide(c, k.N, k.mDescriptors, k.angles);
        r.has_point = k.hasPoint;
        r.n_left = k.NLeft;
        r.n_un = k.nUn;
        return r;
    };
    const ft_bow_keyframe K1 = record(kf1, csr[nn]);
    std::vector<ft_bow_keyframe> K2(nn);
    for (size_t k = 0; k < nn; k++) K2[k] = record(kf2s[k], csr[k]);
    std::vector<int> flat(nn * n1 + 1, -1), nmatches(nn + 1, 0);
    check(ft_search_by_bow_keyframes(ctx.handle(), &K1, (int)nn, K2.data(), nnRatio, checkOrientation ? 1 : 0, flat.data(), nmatches.data()));
    vvMatches12.assign(nn, {});
    for (size_t k = 0; k < nn; k++) vvMatches12[k].assign(flat.begin() + k * n1, flat.begin() + (k + 1) * n1);
    nmatches.resize(nn);
    return nmatches;
}

// What ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, vpMapPointMatches) reads of a candidate KeyFrame: mFeatVec, mDescriptors
// (N rows), hasPoint[i] = GetMapPoint(i) && !GetMapPoint(i)->isBad(), angles = cv::KeyPoint::angle per feature (the right
// camera's after the left one's).
struct BowCandidate {
    const ORBVocabulary::FeatureVector *mFeatVec = nullptr;
    const uint8_t *mDescriptors = nullptr;
    int N = 0;
    const uint8_t *hasPoint = nullptr;
    const float *angles = nullptr;
};
// ORBmatcher(nnRatio, checkOrientation).SearchByBoW(vpCandidateKFs[k], F, vvpMapPointMatches[k]) for the frame against every
// candidate in one call (ft_search_by_bow_candidates; the loop of Tracking::Relocalization, src/Tracking.cc:3839-3860, whose
// isBad() test on the candidates stays with the caller).  fDescriptorsOnDevice: fDescriptors is a device pointer, read in place.
// vvMatches[k][i] = index into candidates[k]'s GetMapPointMatches() or -1:
// `vvpMapPointMatches[k][i] = m < 0 ? nullptr : vpMapPointsKF[m]`.  Returns nmatches per candidate.
inline std::vector<int> SearchByBoW(Context &ctx, const std::vector<BowCandidate> &candidates, const ORBVocabulary::FeatureVector &fFeatVec,
                                    const uint8_t *fDescriptors, int fN, const float *fAngles, int fNleft, bool fDescriptorsOnDevice,
                                    float nnRatio, bool checkOrientation, std::vector<std::vector<int>> &vvMatches) {
    const size_t nk = candidates.size(), nf = fN > 0 ? (size_t)fN : 0;
    std::vector<detail::BowCsr> csr(nk + 1);
    csr[nk] = detail::flattenFeatVec(fFeatVec);
    const ft_bow_side F = detail::bowSide(csr[nk], fN, fDescriptors, fAngles);
    std::vector<ft_bow_candidate> K(nk);
    for (size_t k = 0; k < nk; k++) {
        if (!candidates[k].mFeatVec) throw std::invalid_argument("SearchByBoW: a candidate without mFeatVec");
        csr[k] = detail::flattenFeatVec(*candidates[k].mFeatVec);
        K[k].side = detail::bowSide(csr[k], candidates[k].N, candidates[k].mDescriptors, candidates[k].angles);
        K[k].has_point = candidates[k].hasPoint;
    }
    std::vector<int> flat(nk * nf + 1, -1), nmatches(nk + 1, 0);
    check(ft_search_by_bow_candidates(ctx.handle(), &F, fNleft, fDescriptorsOnDevice ? 1 : 0, (int)nk, K.data(), nnRatio,
                                      checkOrientation ? 1 : 0, flat.data(), nmatches.data()));
    vvMatches.assign(nk, {});
    for (size_t k = 0; k < nk; k++) vvMatches[k].assign(flat.begin() + k * nf, flat.begin() + (k + 1) * nf);
    nmatches.resize(nk);
    return nmatches;
}

// ORBmatcher(0.6, mbCheckOrientation).SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse)
// (src/ORBmatcher.cc:1006-1245) for pKF1 against every neighbour of LocalMapping::CreateNewMapPoints in one call
// (ft_search_for_triangulation): vpKF2 are the neighbours that passed the caller's baseline filter, vPairs the constants of each
// pair (ep, F12 or R12 / t12).  vMatchedPairs[k] is the reference's vMatchedPairs against vpKF2[k], the return
// value its nmatches per neighbour.
inline std::vector<int> SearchForTriangulation(Context &ctx, const ft_triang_keyframe &pKF1, const std::vector<ft_triang_keyframe> &vpKF2,
                                               const std::vector<ft_triang_pair> &vPairs, bool bOnlyStereo, bool bCoarse,
                                               bool mbCheckOrientation,
                                               std::vector<std::vector<std::pair<size_t, size_t>>> &vMatchedPairs) {
    const size_t nn = vpKF2.size(), n1 = pKF1.n > 0 ? (size_t)pKF1.n : 0;
    if (vPairs.size() != nn) throw std::invalid_argument("SearchForTriangulation: one ft_triang_pair per neighbour");
    std::vector<int> vMatches12(nn * n1 + 1, -1), nmatches(nn + 1, 0);
    check(ft_search_for_triangulation(ctx.handle(), &pKF1, (int)nn, vpKF2.data(), vPairs.data(), bOnlyStereo ? 1 : 0, bCoarse ? 1 : 0,
                                      mbCheckOrientation ? 1 : 0, vMatches12.data(), nmatches.data(), nullptr));
    vMatchedPairs.assign(nn, {});
    for (size_t k = 0; k < nn; k++) {
        vMatchedPairs[k].reserve(nmatches[k] > 0 ? (size_t)nmatches[k] : 0);
        for (size_t i = 0; i < n1; i++)
            if (vMatches12[k * n1 + i] >= 0) vMatchedPairs[k].push_back(std::make_pair(i, (size_t)vMatches12[k * n1 + i]));
    }
    nmatches.resize(nn);
    return nmatches;
}

// A point LocalMapping::CreateNewMapPoints would create (src/LocalMapping.cc:694): the pair, x3D and bPointStereo
struct NewMapPoint {
    size_t idx1, idx2;
    float x3D[3];
    bool bPointStereo;
};
namespace detail {
inline std::vector<std::vector<NewMapPoint>> newMapPoints(size_t nn, size_t n1, const std::vector<int> &matches12, const std::vector<int> &status,
                                                          const std::vector<float> &x3d) {
    std::vector<std::vector<NewMapPoint>> out(nn);
    for (size_t k = 0; k < nn; k++)
        for (size_t i = 0; i < n1; i++) {
            const size_t s = k * n1 + i;
            if (status[s] <= 0) continue;
            out[k].push_back(NewMapPoint{i, (size_t)matches12[s], {x3d[3 * s], x3d[3 * s + 1], x3d[3 * s + 2]}, status[s] != 1});
        }
    return out;
}
}  // namespace detail

// The triangulation loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:483-692) on the vMatchedPairs of every neighbour
// (ft_triangulate_new_points): mbInertial, mbFarPoints, mThFarPoints, ratioFactor = 1.5f * mfScaleFactor.  Returns per neighbour the
// accepted points in ascending idx1; firstNeighbour[idx1] (if asked for) is the neighbour whose point the reference's loop attaches
// to idx1, -1 = none (see the loop-order note in fasttrack_amd.h).
inline std::vector<std::vector<NewMapPoint>> TriangulateNewPoints(Context &ctx, const ft_triang_keyframe &pKF1, const ft_newpoint_geometry &g1,
                                                                  const std::vector<ft_triang_keyframe> &vpKF2,
                                                                  const std::vector<ft_newpoint_geometry> &vg2,
                                                                  const std::vector<std::vector<std::pair<size_t, size_t>>> &vMatchedPairs,
                                                                  bool mbInertial, bool mbFarPoints, float mThFarPoints, float ratioFactor,
                                                                  std::vector<int> *firstNeighbour = nullptr) {
    const size_t nn = vpKF2.size(), n1 = pKF1.n > 0 ? (size_t)pKF1.n : 0;
    if (vg2.size() != nn || vMatchedPairs.size() != nn) throw std::invalid_argument("TriangulateNewPoints: one geometry and one pair list per neighbour");
    std::vector<int> matches12(nn * n1 + 1, -1), status(nn * n1 + 1, 0), nPoints(nn + 1, 0), first(n1 + 1, -1);
    std::vector<float> x3d(3 * (nn * n1 + 1), 0.f);
    for (size_t k = 0; k < nn; k++)
        for (const auto &m : vMatchedPairs[k]) {
            if (m.first >= n1) throw std::invalid_argument("TriangulateNewPoints: idx1 out of range");
            matches12[k * n1 + m.first] = (int)m.second;
        }
    check(ft_triangulate_new_points(ctx.handle(), &pKF1, &g1, (int)nn, vpKF2.data(), vg2.data(), matches12.data(), mbInertial ? 1 : 0,
                                    mbFarPoints ? 1 : 0, mThFarPoints, ratioFactor, status.data(), x3d.data(), nPoints.data(), first.data()));
    if (firstNeighbour) firstNeighbour->assign(first.begin(), first.begin() + n1);
    return detail::newMapPoints(nn, n1, matches12, status, x3d);
}

// SearchForTriangulation and the loop above in one call (ft_search_and_triangulate): the matches stay on the device in between.
inline std::vector<std::vector<NewMapPoint>> SearchAndTriangulate(Context &ctx, const ft_triang_keyframe &pKF1, const ft_newpoint_geometry &g1,
                                                                  const std::vector<ft_triang_keyframe> &vpKF2,
                                                                  const std::vector<ft_newpoint_geometry> &vg2,
                                                                  const std::vector<ft_triang_pair> &vPairs, bool bOnlyStereo, bool bCoarse,
                                                                  bool mbCheckOrientation, bool mbInertial, bool mbFarPoints, float mThFarPoints,
                                                                  float ratioFactor, std::vector<int> *firstNeighbour = nullptr,
                                                                  std::vector<int> *nmatches = nullptr) {
    const size_t nn = vpKF2.size(), n1 = pKF1.n > 0 ? (size_t)pKF1.n : 0;
    if (vg2.size() != nn || vPairs.size() != nn) throw std::invalid_argument("SearchAndTriangulate: one geometry and one ft_triang_pair per neighbour");
    std::vector<int> matches12(nn * n1 + 1, -1), status(nn * n1 + 1, 0), nPoints(nn + 1, 0), first(n1 + 1, -1), nm(nn + 1, 0);
    std::vector<float> x3d(3 * (nn * n1 + 1), 0.f);
    check(ft_search_and_triangulate(ctx.handle(), &pKF1, &g1, (int)nn, vpKF2.data(), vg2.data(), vPairs.data(), bOnlyStereo ? 1 : 0,
                                    bCoarse ? 1 : 0, mbCheckOrientation ? 1 : 0, mbInertial ? 1 : 0, mbFarPoints ? 1 : 0, mThFarPoints, ratioFactor,
                                    matches12.data(), nm.data(), nullptr, status.data(), x3d.data(), nPoints.data(), first.data()));
    if (firstNeighbour) firstNeighbour->assign(first.begin(), first.begin() + n1);
    if (nmatches) nmatches->assign(nm.begin(), nm.begin() + nn);
    return detail::newMapPoints(nn, n1, matches12, status, x3d);
}

// Optimizer::PoseOptimization(Frame *pFrame) (src/Optimizer.cc:814-1114) for a batch of independent frames in one launch
// (ft_pose_optimization).  vFrames: what the optimisation reads of each Frame; mvbOutlier[f] is resized to the frame's N (new
// entries false) and keeps its entries without a map point; vPoses[f] is the optimised pose (pFrame->SetPose).  Returns per frame
// nInitialCorrespondences - nBad.  The sweep behind the call (src/Tracking.cc:2992-3020) stays with the caller.
inline std::vector<int> PoseOptimization(Context &ctx, const std::vector<ft_pose_opt_frame> &vFrames, std::vector<ft_se3> &vPoses,
                                         std::vector<std::vector<uint8_t>> &mvbOutlier, std::vector<ft_pose_opt_trace> *trace = nullptr) {
    const size_t n = vFrames.size();
    vPoses.resize(n);
    mvbOutlier.resize(n);
    std::vector<uint8_t *> flags(n + 1, nullptr);
    for (size_t f = 0; f < n; f++) {
        mvbOutlier[f].resize(vFrames[f].N > 0 ? (size_t)vFrames[f].N : 0, 0);
        flags[f] = mvbOutlier[f].data();
    }
    std::vector<int> inliers(n + 1, 0);
    if (trace) trace->assign(n, ft_pose_opt_trace{});
    check(ft_pose_optimization(ctx.handle(), (int)n, vFrames.data(), vPoses.data(), flags.data(), inliers.data(), trace ? trace->data() : nullptr));
    inliers.resize(n);
    return inliers;
}

// Sim3Solver (src/Sim3Solver.cc) for the candidates of a keyframe in one call (ft_sim3_solver): per problem what
//   Sim3Solver solver(pKF1, pKF2, vpMatched12, bFixScale, vpKeyFrameMatchedMP); solver.SetRansacParameters(p, minInliers, maxIts);
//   while (!bConverge && !bNoMore) mTcm = solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge);
// (src/LoopClosing.cc:698-710) leaves behind.  results[p] onto the out-parameters: bNoMore = no_more, bConverge = converged,
// nInliers = n_inliers, mTcm = T12 (row-major Matrix4f); onto the getters: GetEstimatedRotation() = R (row-major),
// GetEstimatedTranslation() = t, GetEstimatedScale() = s, so that gScm = g2o::Sim3(R, t, s) as at :746; mnBestInliers =
// n_best_inliers.  vbInliers[p] is resized to the problem's n and holds iterate's vbInliers; bestInliers (may be null) receives
// mvbBestInliers, hypothesisInliers (may be null) mnInliersi of every evaluated iteration (effective_iterations entries).
inline void Sim3SolverBatch(Context &ctx, const std::vector<ft_sim3_problem> &vProblems, std::vector<ft_sim3_result> &results,
                            std::vector<std::vector<uint8_t>> &vbInliers, std::vector<std::vector<uint8_t>> *bestInliers = nullptr,
                            std::vector<std::vector<int>> *hypothesisInliers = nullptr) {
    const size_t n = vProblems.size();
    results.assign(n + 1, ft_sim3_result{});
    vbInliers.resize(n);
    if (bestInliers) bestInliers->resize(n);
    if (hypothesisInliers) hypothesisInliers->resize(n);
    std::vector<uint8_t *> in(n + 1, nullptr), best(n + 1, nullptr);
    std::vector<int *> hyp(n + 1, nullptr);
    for (size_t p = 0; p < n; p++) {
        const size_t np = vProblems[p].n > 0 ? (size_t)vProblems[p].n : 0;
        vbInliers[p].assign(np + 1, 0);
        in[p] = vbInliers[p].data();
        if (bestInliers) (*bestInliers)[p].assign(np + 1, 0), best[p] = (*bestInliers)[p].data();
        if (hypothesisInliers)
            (*hypothesisInliers)[p].assign(vProblems[p].max_iterations > 0 ? (size_t)vProblems[p].max_iterations : 1, 0), hyp[p] = (*hypothesisInliers)[p].data();
    }
    check(ft_sim3_solver(ctx.handle(), (int)n, vProblems.data(), results.data(), in.data(), bestInliers ? best.data() : nullptr,
                         hypothesisInliers ? hyp.data() : nullptr));
    results.resize(n);
    for (size_t p = 0; p < n; p++) {
        vbInliers[p].pop_back();
        if (bestInliers) (*bestInliers)[p].pop_back();
        if (hypothesisInliers) (*hypothesisInliers)[p].resize((size_t)results[p].effective_iterations);
    }
}

// ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) (src/ORBmatcher.cc:1247-1437) and Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
// (:1439-1554) for one list of map points against every target (keyframe, camera) of LocalMapping::SearchInNeighbors or
// LoopClosing::SearchAndFuse in one call (ft_fuse_search).  vpMapPoints are the arrays of the points, vTargets one record per
// Fuse call of the reference's loop (check_reprojection = 1 for the SE3 overload, 0 for the Sim3 one).  bestIdx[k][i] / bestDist[k][i]
// are the loop's bestIdx / bestDist of point i against target k (-1 / 256: none); the return value counts, per target, the points
// with bestDist <= TH_LOW.  The bookkeeping behind the loop stays with the caller (INTEGRATION.md has the apply loop).
inline std::vector<int> Fuse(Context &ctx, const ft_fuse_points &vpMapPoints, const std::vector<ft_fuse_target> &vTargets,
                             std::vector<std::vector<int>> &bestIdx, std::vector<std::vector<int>> &bestDist,
                             std::vector<std::vector<uint8_t>> *stage = nullptr) {
    const size_t nt = vTargets.size(), M = vpMapPoints.M > 0 ? (size_t)vpMapPoints.M : 0;
    std::vector<int> idx(nt * M + 1, -1), dist(nt * M + 1, 256), nFound(nt + 1, 0);
    std::vector<uint8_t> st(stage ? nt * M + 1 : 0, 0);
    check(ft_fuse_search(ctx.handle(), &vpMapPoints, (int)nt, vTargets.data(), idx.data(), dist.data(), stage ? st.data() : nullptr,
                         nFound.data()));
    bestIdx.assign(nt, {});
    bestDist.assign(nt, {});
    if (stage) stage->assign(nt, {});
    for (size_t k = 0; k < nt; k++) {
        bestIdx[k].assign(idx.begin() + k * M, idx.begin() + (k + 1) * M);
        bestDist[k].assign(dist.begin() + k * M, dist.begin() + (k + 1) * M);
        if (stage) (*stage)[k].assign(st.begin() + k * M, st.begin() + (k + 1) * M);
    }
    nFound.resize(nt);
    return nFound;
}

// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (src/ORBmatcher.cc:526-631) on arrays
// (ft_search_keyframe_sim3 with one job).  Scw is what the reference derives from it: Tcw = SE3f(Scw.rotationMatrix(),
// Scw.translation() / Scw.scale()) and Ow = Tcw.inverse().translation(); vpPoints the arrays of the points with valid[i] =
// !isBad() && !spAlreadyFound.count(pMP) (NULL: all); vpMatched holds point indices, -1 = NULL, and receives the index of every
// point that wrote.  pointKeypoint (may be null) receives the keypoint every point wrote, or -1.  Returns nmatches.
struct Sim3Pose {
    ft_se3 Tcw;
    float Ow[3];
    float logScaleFactor;  // pKF->mfLogScaleFactor
};
inline int SearchByProjection(Context &ctx, const ft_frame_view &pKF, const Sim3Pose &Scw, const ft_fuse_points &vpPoints, const uint8_t *valid,
                              std::vector<int> &vpMatched, int th, float ratioHamming, std::vector<int> *pointKeypoint = nullptr,
                              int handPinhole = 0) {
    ft_sim3_job job = {};
    job.points = vpPoints;
    job.valid = valid;
    job.Tcw = Scw.Tcw;
    for (int k = 0; k < 3; k++) job.Ow[k] = Scw.Ow[k];
    job.log_scale_factor = Scw.logScaleFactor;
    job.th = th;
    job.ratio_hamming = ratioHamming;
    job.hand_pinhole = handPinhole;
    vpMatched.resize(pKF.N > 0 ? (size_t)pKF.N : 0, -1);
    std::vector<int> none(1, -1);
    job.matched = vpMatched.empty() ? none.data() : vpMatched.data();
    if (pointKeypoint) {
        pointKeypoint->assign(vpPoints.M > 0 ? (size_t)vpPoints.M : 0, -1);
        job.point_keypoint = pointKeypoint->empty() ? nullptr : pointKeypoint->data();
    }
    check(ft_search_keyframe_sim3(ctx.handle(), &pKF, 1, &job));
    return job.n_matches;
}

// The overload with vpPointsKFs / vpMatchedKF (:633-745): the projection written out by hand, and vpMatchedKF[idx] = vpPointsKFs[iMP]
// for every keypoint a point wrote - filled here from the keypoint each point reports.  KF is whatever the caller keeps per point.
template <class KF>
inline int SearchByProjection(Context &ctx, const ft_frame_view &pKF, const Sim3Pose &Scw, const ft_fuse_points &vpPoints, const uint8_t *valid,
                              const std::vector<KF> &vpPointsKFs, std::vector<int> &vpMatched, std::vector<KF> &vpMatchedKF, int th,
                              float ratioHamming) {
    std::vector<int> pointKeypoint;
    const int nmatches = SearchByProjection(ctx, pKF, Scw, vpPoints, valid, vpMatched, th, ratioHamming, &pointKeypoint, 1);
    vpMatchedKF.resize(vpMatched.size());
    for (size_t i = 0; i < pointKeypoint.size() && i < vpPointsKFs.size(); i++)
        if (pointKeypoint[i] >= 0) vpMatchedKF[(size_t)pointKeypoint[i]] = vpPointsKFs[i];
    return nmatches;
}

// Every search a caller has against one keyframe in one call: the loop and the merge detection of NewDetectCommonRegions, the
// candidates of DetectCommonRegionsFromBoW (the jobs' matched / point_keypoint / stage / n_matches are written in place).
inline void SearchByProjection(Context &ctx, const ft_frame_view &pKF, std::vector<ft_sim3_job> &vJobs) {
    check(ft_search_keyframe_sim3(ctx.handle(), &pKF, (int)vJobs.size(), vJobs.data()));
}

// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:329-403) for every map point of a loop in one call
// (ft_distinctive_descriptors): the loops of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:312-323), SearchInNeighbors
// (:806-816) and CreateNewMapPoints (:704).  vvDescriptors[p] = the point's vDescriptors as row pointers, in the order the loop at
// :348-363 pushes them (`pKF->mDescriptors.ptr(leftIndex)`, then `ptr(rightIndex)`, bad keyframes skipped); a list holds at most
// FT_DISTINCT_MAX_OBSERVATIONS rows.  mDescriptors[p] receives vDescriptors[BestIdx] (:401); the entry of a point with an empty list
// is left as it is (the reference returns at :365) - the vector is resized to the number of points, its entries are kept.
// Returns BestIdx per point (-1 for an empty list); bestMedian, when given, BestMedian (-1).
typedef std::array<uint8_t, 32> Descriptor256;
inline std::vector<int> ComputeDistinctiveDescriptors(Context &ctx, const std::vector<std::vector<const uint8_t *>> &vvDescriptors,
                                                      std::vector<Descriptor256> &mDescriptors, std::vector<int> *bestMedian = nullptr) {
    const size_t np = vvDescriptors.size();
    std::vector<int> offsets(np + 1, 0);
    for (size_t p = 0; p < np; p++) offsets[p + 1] = offsets[p] + (int)vvDescriptors[p].size();
    std::vector<uint8_t> rows((size_t)offsets[np] * 32 + 1);
    size_t r = 0;
    for (const std::vector<const uint8_t *> &v : vvDescriptors)
        for (const uint8_t *d : v) std::memcpy(rows.data() + 32 * r++, d, 32);
    mDescriptors.resize(np);
    std::vector<int> bestIdx(np + 1, -1);
    if (bestMedian) bestMedian->assign(np + 1, -1);
    check(ft_distinctive_descriptors(ctx.handle(), (int)np, offsets.data(), rows.data(), bestIdx.data(),
                                     bestMedian ? bestMedian->data() : nullptr,
                                     np ? reinterpret_cast<uint8_t *>(mDescriptors.data()) : nullptr));
    bestIdx.resize(np);
    if (bestMedian) bestMedian->resize(np);
    return bestIdx;
}

// KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) resident on the device (ft_kfdb_*): add, erase, clear,
// DetectNBestCandidates (:604-730) and DetectRelocalizationCandidates (:733-845), the two queries with a caller.  A keyframe is
// known by the handle add returns (keep it beside the KeyFrame*: `int mnDatabaseHandle`).  mnPlaceRecognitionQuery / Words /
// Score and the mnReloc* set live in the database and persist between queries, as they do in the KeyFrame.  What the queries
// read from host state that changes between them comes in through two callbacks, asked for the SCORED keyframes only:
//   neighbours(handle) = the handles of pKFi->GetBestCovisibilityKeyFrames(10), in that order;
//   mapOf(handle)      = an integer label of pKFi->GetMap() (the map's mnId).
// KeyFrame::SetBadFlag erases (KeyFrame.cc:678), so the database holds no bad keyframe and the isBad() test of :712 has no
// counterpart; clearMap(pMap) (:74-98) is erase() of that map's handles.
class KeyFrameDatabase {
public:
    typedef std::function<std::vector<int>(int)> NeighboursFn;
    typedef std::function<int(int)> MapFn;
    explicit KeyFrameDatabase(Context &ctx, int scoring = 0) { check(ft_kfdb_create(ctx.handle(), scoring, &h_)); }
    ~KeyFrameDatabase() { ft_kfdb_destroy(h_); }
    KeyFrameDatabase(const KeyFrameDatabase &) = delete;
    KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;
    ft_kfdb *handle() const { return h_; }

    // void add(KeyFrame *pKF): pKF->mBowVec -> the keyframe's handle
    int add(const ORBVocabulary::BowVector &mBowVec) {
        std::vector<unsigned> ids;
        std::vector<double> values;
        flatten(mBowVec, ids, values);
        const int offsets[2] = {0, (int)ids.size()};
        int handle = -1;
        check(ft_kfdb_add(h_, 1, offsets, ids.data(), values.data(), &handle));
        return handle;
    }
    void erase(int handle) { check(ft_kfdb_erase(h_, 1, &handle)); }
    void erase(const std::vector<int> &handles) { check(ft_kfdb_erase(h_, (int)handles.size(), handles.data())); }  // clearMap
    void clear() { check(ft_kfdb_clear(h_)); }
    int size() const {
        int n = 0;
        check(ft_kfdb_size(h_, &n, nullptr));
        return n;
    }

    // void DetectNBestCandidates(KeyFrame *pKF, vector<KeyFrame*> &vpLoopCand, vector<KeyFrame*> &vpMergeCand, int nNumCandidates):
    // pKF as mnId, mBowVec, the handles of GetConnectedKeyFrames() and the label of GetMap(); badMaps: labels of maps with IsBad()
    void DetectNBestCandidates(long long mnId, const ORBVocabulary::BowVector &mBowVec, const std::vector<int> &vConnected, int map,
                               const NeighboursFn &neighbours, const MapFn &mapOf, std::vector<int> &vpLoopCand,
                               std::vector<int> &vpMergeCand, int nNumCandidates, const std::vector<int> &badMaps = {}) {
        Scored s = score(FT_KFDB_PLACE_RECOGNITION, mnId, mBowVec, vConnected);
        gather(s, neighbours, mapOf);
        vpLoopCand.assign((size_t)std::max(nNumCandidates, 1), -1);
        vpMergeCand.assign((size_t)std::max(nNumCandidates, 1), -1);
        int nLoop = 0, nMerge = 0;
        check(ft_kfdb_select_n_best(h_, mnId, (int)s.handles.size(), s.handles.data(), s.scores.data(), s.offsets.data(), s.neigh.data(),
                                    s.maps.data(), s.neighMaps.data(), map, (int)badMaps.size(), badMaps.data(), nNumCandidates,
                                    vpLoopCand.data(), &nLoop, vpMergeCand.data(), &nMerge));
        vpLoopCand.resize(nLoop);
        vpMergeCand.resize(nMerge);
    }

    // vector<KeyFrame*> DetectRelocalizationCandidates(Frame *F, Map *pMap): F as mnId and mBowVec
    std::vector<int> DetectRelocalizationCandidates(long long mnId, const ORBVocabulary::BowVector &mBowVec, int map,
                                                    const NeighboursFn &neighbours, const MapFn &mapOf) {
        Scored s = score(FT_KFDB_RELOCALIZATION, mnId, mBowVec, {});
        gather(s, neighbours, mapOf);
        std::vector<int> out(s.handles.size() + 1, -1);
        int n = 0;
        check(ft_kfdb_select_reloc(h_, mnId, (int)s.handles.size(), s.handles.data(), s.scores.data(), s.offsets.data(), s.neigh.data(),
                                   s.maps.data(), s.neighMaps.data(), map, out.data(), &n));
        out.resize(n);
        return out;
    }

private:
    struct Scored {
        std::vector<int> handles, words, offsets, neigh, maps, neighMaps;
        std::vector<float> scores;
    };
    static void flatten(const ORBVocabulary::BowVector &v, std::vector<unsigned> &ids, std::vector<double> &values) {
        ids.reserve(v.size() + 1);
        values.reserve(v.size() + 1);
        for (const auto &e : v) ids.push_back(e.first), values.push_back(e.second);
    }
    Scored score(int kind, long long mnId, const ORBVocabulary::BowVector &mBowVec, const std::vector<int> &vConnected) {
        std::vector<unsigned> ids;
        std::vector<double> values;
        flatten(mBowVec, ids, values);
        Scored s;
        const size_t room = (size_t)size() + 1;
        s.handles.resize(room);
        s.words.resize(room);
        s.scores.resize(room);
        int nSharing = 0, maxWords = 0, minWords = 0, nScored = 0;
        check(ft_kfdb_score(h_, kind, mnId, (int)ids.size(), ids.data(), values.data(), (int)vConnected.size(), vConnected.data(),
                            &nSharing, &maxWords, &minWords, &nScored, s.handles.data(), s.words.data(), s.scores.data(), nullptr));
        s.handles.resize(nScored);
        s.words.resize(nScored);
        s.scores.resize(nScored);
        return s;
    }
    static void gather(Scored &s, const NeighboursFn &neighbours, const MapFn &mapOf) {
        s.offsets.assign(1, 0);
        for (int h : s.handles) {
            for (int h2 : neighbours(h)) s.neigh.push_back(h2), s.neighMaps.push_back(mapOf(h2));
            s.offsets.push_back((int)s.neigh.size());
            s.maps.push_back(mapOf(h));
        }
        s.neigh.push_back(-1);  // (never read: data() of an empty vector may be null)
        s.neighMaps.push_back(-1);
        s.maps.push_back(-1);
    }
    ft_kfdb *h_ = nullptr;
};

}  // namespace fasttrack
