/*
 * fasttrack_amd.h - C ABI of the MI355X-native ORB tracking front end.
 *
 * This is the drop-in boundary: every entry point replaces one seam of the reference
 * (sfu-rsl/FastTrack, paths relative to its root) and takes plain pointers and sizes only - no
 * OpenCV / Eigen / torch types - so it binds from C++, C or ctypes alike.  INTEGRATION.md shows the
 * adapter a maintainer adds on the ORB-SLAM3 side.
 *
 * Conventions
 *  - every function returns FT_OK (0) or a negative ft_status; ft_last_error() returns the message of
 *    the calling thread's last failure (the reference prints and exit()s: src/Kernels/CudaUtils.cu:17-22).
 *  - handles are bound to one device; calls on different handles are re-entrant (the reference calls
 *    the left and right extractor from two host threads: src/Frame.cc:127-130); calls on the same
 *    handle must be serialised by the caller.
 *  - all compute runs in hand-written HIP kernels on the handle's device.  There is no CPU fallback:
 *    without a usable gfx950 device every compute entry point fails with FT_ERR_NO_DEVICE.
 *  - ft_keypoint has the field order and size (28 B) of cv::KeyPoint, so a std::vector<cv::KeyPoint>
 *    can be passed as ft_keypoint* directly.
 */
#ifndef FASTTRACK_AMD_H
#define FASTTRACK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FT_API __attribute__((visibility("default")))

typedef enum ft_status {
    FT_OK = 0,
    FT_ERR_INVALID = -1,   /* bad argument */
    FT_ERR_NO_DEVICE = -2, /* no usable HIP device / extension not functional */
    FT_ERR_HIP = -3,       /* a HIP runtime call failed */
    FT_ERR_CAPACITY = -4,  /* caller buffer too small */
    FT_ERR_EMPTY = -5      /* empty input image (ORBextractor::operator() returns -1, ORBextractor.cc:1360) */
} ft_status;

/* cv::KeyPoint layout: pt.x pt.y size angle response octave class_id */
typedef struct ft_keypoint {
    float x, y, size, angle, response;
    int octave, class_id;
} ft_keypoint;

/* ------------------------------------------------------------------------------------------------
 * Library / device context.
 * Replaces KernelController::setCUDADevice / initializeKernels / shutdownKernels / saveKernelsStats
 * (include/Kernels/KernelController.h:15-29) and CudaUtils::loadSetting (include/Kernels/CudaUtils.h:21).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_context ft_context;

FT_API const char *ft_version(void);
FT_API const char *ft_last_error(void);
FT_API int ft_device_count(void); /* number of HIP devices, 0 if none (never fails) */
/* PCI bus id ("0000:c1:00.0") of a device: /sys/bus/pci/devices/<id>/numa_node names the host memory node next to it, so a
 * process that serves one GPU (reference: one KernelController per process, src/Kernels/KernelController.cu:24-29) can pin
 * its host threads there before it creates the context */
FT_API int ft_device_pci_bus_id(int device, char *buf, int len);
/* host_threads: workers for the host-side octree stage (0 = the CPUs this process may use:
 * hardware threads capped by affinity and by a cgroup CPU quota).
 * No side effects on the process environment.  Extractors for batches of more than 16 frames run on streams of the context
 * ("lanes") by a table made for the number of hardware queues the HIP runtime gives the process: GPU_MAX_HW_QUEUES, which
 * the runtime reads ONCE, at the first HIP call of the process.  An application that wants the eight-lane table (+10 % on
 * the headline workload over the four queues of the runtime's default) sets GPU_MAX_HW_QUEUES=10 before its first HIP call
 * (INTEGRATION.md section 6); ft_context_hw_queues() reports what the context was created under (4 = variable unset).
 * FT_LANE_MAP ("own" or whole sets of four lane numbers) overrides the table; a malformed value is FT_ERR_INVALID.
 * ft_context_destroy refuses (FT_ERR_INVALID) while extractors, front ends or tracked frames of the context are alive:
 * they run on its streams. */
FT_API int ft_context_create(int device, int host_threads, ft_context **out);
FT_API int ft_context_destroy(ft_context *ctx);
FT_API int ft_context_synchronize(ft_context *ctx);
FT_API int ft_context_device_name(ft_context *ctx, char *buf, int len);
FT_API int ft_context_hw_queues(const ft_context *ctx);
/* The lane table of the extractors created on the context from now on: n = 4 * sets entries, (stage A, stage B, octree 0,
 * octree 1) lane numbers in [0, 64) for the 1st, 2nd, ... extractor (wrapping around); n = 0: private streams for every
 * extractor.  What FT_LANE_MAP does through the environment; tools/lane_search.py finds a table for a given stream of frames. */
FT_API int ft_context_set_lane_map(ft_context *ctx, const int *map, int n);
/* Tuning options.  Every switch of the library that is not a debugging aid is a named integer option of the CONTEXT.
 * ft_context_create reads the initial values from the environment, once (variable = "FT_" + upper-case name):
 *
 *   name                 default  range    meaning
 *   pipeline_depth       0        0 .. 8   sub-batches a throughput batch is enqueued as (0 = automatic, 1 = no pipelining)
 *   device_octree        1        0 .. 1   DistributeOctTree on the device (0 = host thread pool)
 *   oct_hist             1        0 .. 1   histogram tier of the device octree for levels above 4096 candidates
 *   oct_hist_first       1        0 .. 2   histogram formulation for every level: 0 never, 1 latency-mode launches, 2 always
 *   oct_big              1        0 .. 1   sorted big tier of the device octree (up to 16384 keys per level)
 *   pyr_rows             2        0 .. 2   pyramid of launches of 8+ images: 2 = all levels in one launch, a workgroup per band
 *                                          of an image (a per-level loop of the row-streaming kernel where a level does not fit
 *                                          it), 1 = row-streaming kernel, a launch per level, 0 = tile kernel
 *   upload_kernel        1        0 .. 1   latency mode: frames go up through one kernel instead of DMA copies
 *   graph                1        0 .. 1   latency mode: batches of <= 8 frames are captured and replayed as HIP graphs
 *   paired               1        0 .. 1   latency-mode stereo front ends run both cameras through one set of launches
 *   pass_burst           12       2 .. 14  projection searches: claim passes enqueued per host round trip
 *   search_cache         2        0 .. 3   projection searches: 1 = later claim passes walk the cached candidate keys; 2 = and a
 *                                          batch of 24 or more frames resolves its claims in one launch behind the first pass (a
 *                                          workgroup per frame); 3 = every batch does
 *   search_grid          1        0 .. 1   projection searches: CSR grid of the frame built on the device
 *   blocking_sync        2        0 .. 2   host waits for the device: 0 = the runtime's default (it spins), 1 = sleeping
 *                                          (hipDeviceScheduleBlockingSync: a waiting thread leaves its core to the others - 10 - 20 us
 *                                          later wake-ups), 2 = sleeping when the process may use fewer than 8 CPUs.  Read by
 *                                          ft_context_create only (a device flag of the whole process)
 *
 * A value outside an option's range is FT_ERR_INVALID (from ft_context_set_option, and from ft_context_create when it comes
 * from the environment).
 * ft_context_set_option changes the context's value; extractors, front ends and tracked frames take the switches of their
 * context when they are CREATED (the search_* and pass_burst options are read per call).  `name` is the option name or its
 * environment spelling.  ft_option_describe enumerates the table (index 0, 1, ... until FT_ERR_INVALID).
 * Only the FT_DEBUG_* aids (FT_DEBUG_REPEAT, FT_DEBUG_OCC, FT_DEBUG_FAST, FT_DEBUG_OD_PROFILE, FT_DEBUG_OCT_PROFILE, and
 * FT_DEBUG_OCTREE_PATHS / _HIST_BINS / _HIST_STRICT of the host test entry ft_octree_distribute) and FT_LANE_MAP are read from
 * the environment anywhere else; none of them changes results. */
FT_API int ft_context_set_option(ft_context *ctx, const char *name, int value);
FT_API int ft_context_get_option(const ft_context *ctx, const char *name, int *value);
FT_API int ft_option_describe(int index, const char **name, const char **env, int *default_value, const char **doc);
FT_API int ft_option_range(const char *name, int *min_value, int *max_value);
FT_API int ft_context_host_threads(const ft_context *ctx);
/* per-stage wall/GPU timings of the calls made so far; the reference's REGISTER_STATS analogue
 * (include/Kernels/CudaUtils.h:14, src/Stats.cc:31-60).  Writes "<name>: <ms>" lines. */
FT_API int ft_context_save_stats(ft_context *ctx, const char *path);
/* kernel timing with HIP events on the launching stream (off by default); names are "kernel.<name>" */
FT_API int ft_context_set_kernel_timing(ft_context *ctx, int enabled);
FT_API int ft_context_get_stat(ft_context *ctx, const char *name, double *total_ms, long *calls);
FT_API int ft_context_reset_stats(ft_context *ctx);
/* device memory helpers so that a caller (or bench.py) can keep frames resident in HBM */
FT_API int ft_device_malloc(ft_context *ctx, size_t bytes, void **dptr);
FT_API int ft_device_free(ft_context *ctx, void *dptr);
/* pinned host memory: result arrays allocated here are filled by the device copies directly.  A block is released by
 * ft_host_free, or with its context: ft_context_destroy frees what is still allocated (do not use such a block afterwards). */
FT_API int ft_host_malloc(ft_context *ctx, size_t bytes, void **ptr);
FT_API int ft_host_free(ft_context *ctx, void *ptr);
FT_API int ft_memcpy_h2d(ft_context *ctx, void *dst, const void *src, size_t bytes);
FT_API int ft_memcpy_d2h(ft_context *ctx, void *dst, const void *src, size_t bytes);

/* ------------------------------------------------------------------------------------------------
 * ORB extractor.  Replaces ORB_SLAM3::ORBextractor (include/ORBextractor.h:100-197):
 *   ctor (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, imageWidth, imageHeight)  :105-106
 *   int operator()(image, mask, keypoints, descriptors, vLappingArea)                       :113-115
 *   GetLevels/GetScaleFactor(s)/GetInverseScaleFactors/GetScaleSigmaSquares/...             :117-144
 *   mvImagePyramid (:146) and GetGPUPyramid() (:126-128)
 * Results equal the reference's CPU branch (KernelController::orbExtractionKernelRunStatus == 0).
 * max_batch image slots are allocated; slot b keeps the pyramid of the b-th image of the last call
 * resident in HBM for the stereo matcher.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_extractor ft_extractor;

FT_API int ft_extractor_create(ft_context *ctx, int nfeatures, float scale_factor, int nlevels, int ini_th_fast,
                               int min_th_fast, int image_width, int image_height, int max_batch,
                               ft_extractor **out);
FT_API int ft_extractor_destroy(ft_extractor *ex);
FT_API int ft_extractor_levels(const ft_extractor *ex);
FT_API int ft_extractor_max_batch(const ft_extractor *ex);
/* upper bound of keypoints operator() can return per image (octree may exceed nfeatures slightly) */
FT_API int ft_extractor_max_keypoints(const ft_extractor *ex);
/* any of the four output arrays may be NULL; each holds nlevels floats */
FT_API int ft_extractor_scale_factors(const ft_extractor *ex, float *scale, float *inv_scale, float *sigma2,
                                      float *inv_sigma2);
FT_API int ft_extractor_features_per_level(const ft_extractor *ex, int *quota);
FT_API int ft_extractor_level_size(const ft_extractor *ex, int level, int *width, int *height);

/* ORBextractor::operator() for one host image (row stride in bytes).  keypoints/descriptors receive
 * up to `capacity` entries laid out exactly as the reference does (ORBextractor.cc:1466-1487):
 * keypoints with x in [lap0, lap1] fill from the back, the others from the front; *n_mono is the
 * reference's return value.  FT_ERR_EMPTY for a null/empty image. */
FT_API int ft_extract(ft_extractor *ex, const uint8_t *image, int width, int height, int stride, int lap0,
                      int lap1, ft_keypoint *keypoints, uint8_t *descriptors, int capacity, int *n_keypoints,
                      int *n_mono);

/* Modes of an extractor / front end, fixed by max_batch at creation: max_batch <= 16 = LATENCY mode - private streams, and a
 * batch of at most 8 frames with a fixed call shape is captured once as a HIP graph and replayed (statistics
 * "extract.graph_launch" / "stereo.graph_launch" count the replays); max_batch > 16 = THROUGHPUT mode - the streams are lanes
 * of the context shared with the other wide extractors, which a capture cannot use, so such an object never takes the graph
 * path, whatever the size of the batch it is handed (FT_LANE_MAP=own gives wide extractors private streams and the graph path
 * back).  A caller that alternates between single frames and large batches creates one object for each. */

/* The same for `batch` <= max_batch images of identical size.  images[b] is a host pointer
 * (on_device = 0) or a device pointer on this context's device (on_device = 1, frames already in HBM).
 * Outputs are host arrays: keypoints[b*capacity + i], descriptors[(b*capacity + i)*32].  Arrays in pinned memory of the
 * context (ft_host_malloc) are written by the device itself, in the order above, for batches of more than eight images (no
 * staging copy and no pass of the host over the keypoints; statistic "extract.delivered_in_order_on_device"); any other
 * array is filled by the host from the library's staging.  The results are the same. */
FT_API int ft_extract_batch(ft_extractor *ex, const uint8_t *const *images, int batch, int on_device, int width,
                            int height, int stride, int lap0, int lap1, ft_keypoint *keypoints,
                            uint8_t *descriptors, int capacity, int *n_keypoints, int *n_mono);

/* mvImagePyramid[level] of slot `slot` copied to host (tight or strided rows) */
FT_API int ft_extractor_download_level(ft_extractor *ex, int slot, int level, uint8_t *dst, int dst_stride);
/* stage tap for parity tests: level `level` of slot `slot` after cv::GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101)
 * (ORBextractor.cc:1456-1457), computed by the blur routines the descriptor kernel applies on the fly (the path itself
 * never materialises a blurred level) */
FT_API int ft_extractor_download_blurred_level(ft_extractor *ex, int slot, int level, uint8_t *dst, int dst_stride);
/* GetGPUPyramid(): device pointer + pitch of one level of one slot */
FT_API int ft_extractor_device_level(ft_extractor *ex, int slot, int level, const uint8_t **dptr, int *pitch);
/* stage taps for parity tests: FAST candidates handed to the octree, in the CPU's emission order,
 * as (x, y, score) triples relative to the level's (minBorderX, minBorderY) (ORBextractor.cc:1196-1198) */
FT_API int ft_extractor_download_candidates(ft_extractor *ex, int slot, int level, int *xys, int capacity,
                                            int *n);

/* stage tap for parity tests: the DEVICE formulation of DistributeOctTree (ORBextractor.cc:660-884) of one level on
 * caller-provided candidates ((x, y, score) triples relative to the level's (minBorderX, minBorderY), any order: the
 * kernels rank them by the reference's emission order themselves).  tiers: bit 1 allows the histogram tier
 * (k_octree_hist), bit 2 the sorted big tier (k_octree_big), bit 3 selects the kernel of latency-mode launches
 * (k_octree_auto: reported as tier 2); *tier = the tier that produced the result (1, 2, 3), 0 = the
 * level is beyond the allowed tiers (the pipeline would repair the image with the host octree).  out_xys: the retained
 * candidates in the reference's result order. */
FT_API int ft_extractor_octree_on_device(ft_extractor *ex, int level, const int *xys, int n, int tiers, int *out_xys,
                                         int capacity, int *n_out, int *tier);

/* Host-only stages, callable without a GPU (they never touch pixels):
 * ft_octree_distribute = ORBextractor::DistributeOctTree (ORBextractor.cc:660-884), the serial stage
 * that stays on the host in both branches of the reference.  xys: n (x, y, score) candidates relative to
 * (minX, minY) in FAST emission order; out_idx receives the retained candidate indices in the
 * reference's result order; *n_out their number (may exceed N by a few, as in the reference).
 * ft_level_geometry = the level / cell-grid / quota arithmetic of ORBextractor.cc:398-465,1120-1134,1499-1500;
 * every output array holds nlevels ints and may be NULL. */
FT_API int ft_octree_distribute(const int *xys, int n, int minX, int maxX, int minY, int maxY, int N, int *out_idx,
                                int capacity, int *n_out);
FT_API int ft_level_geometry(int width, int height, int nfeatures, float scale_factor, int nlevels, int *level_w,
                             int *level_h, int *quota, int *n_cols, int *n_rows, int *w_cell, int *h_cell);
/* The plan of the one-launch pyramid (pyr_rows = 2), host only: an image is cut into `bands` horizontal bands, band k owns rows
 * [k H / bands, (k + 1) H / bands) of every level (H = the level's height); its row range at a level is the hull of those and of
 * the source rows its range one level up is resized from, so a band reads only rows it wrote.  first_row / end_row:
 * [level * bands + band] for levels 1 .. nlevels - 1 (level 0 entries are zero); first == end: the band has nothing at that level. */
FT_API int ft_pyramid_band_plan(int width, int height, float scale_factor, int nlevels, int bands, int *first_row, int *end_row);

/* ------------------------------------------------------------------------------------------------
 * Stereo matching, rectified pinhole pair.
 * Replaces KernelController::launchStereoMatchKernel (include/Kernels/KernelController.h:31-36) as
 * called from Frame::ComputeStereoMatchesGPU (src/Frame.cc:1007-1063); semantics follow the CPU
 * branch Frame::ComputeStereoMatches (src/Frame.cc:835-1005): row-band Hamming search, 11x11 SAD at
 * 11 shifts, parabola fit, and (apply_median_cut != 0) the 1.5*1.4*median SAD cut.
 * The pyramids are those resident in slot `slot` of exL / exR from their last extract call.
 * uright/depth: mvuRight / mvDepth (-1 = no match); sad (may be NULL): best SAD of kept matches, -1 else.
 * ---------------------------------------------------------------------------------------------- */
FT_API int ft_stereo_match(ft_extractor *exL, ft_extractor *exR, int slot, const ft_keypoint *keysL, int nL,
                           const ft_keypoint *keysR, int nR, const uint8_t *descL, const uint8_t *descR,
                           float mbf, float mb, int apply_median_cut, float *uright, float *depth, int *sad,
                           int *n_matches);

/* Fused stereo front end for throughput: extract left + right and stereo-match `batch` pairs with
 * keypoints and descriptors kept on the device between the stages (one stream per GPU).
 * Outputs per pair b (host arrays, `capacity` entries per image): keysL/descL/keysR/descR as
 * ft_extract_batch, uright/depth for the left keypoints. */
typedef struct ft_stereo_frontend ft_stereo_frontend;
FT_API int ft_stereo_frontend_create(ft_context *ctx, int nfeatures, float scale_factor, int nlevels,
                                     int ini_th_fast, int min_th_fast, int image_width, int image_height,
                                     int max_batch, float mbf, float mb, ft_stereo_frontend **out);
FT_API int ft_stereo_frontend_destroy(ft_stereo_frontend *fe);
FT_API ft_extractor *ft_stereo_frontend_left(ft_stereo_frontend *fe);
FT_API ft_extractor *ft_stereo_frontend_right(ft_stereo_frontend *fe);
/* Asynchronous halves of ft_stereo_frontend_process: submit enqueues everything (it returns once the host
 * octree of the last sub-batch is done and its kernels are queued), wait drains the device and finishes
 * the outputs.  With two front ends used alternately the drain of one batch overlaps with the next batch:
 *   submit(fe[k & 1], batch k);  wait(fe[(k - 1) & 1]);
 * Output arrays of a submitted batch must stay untouched until its wait returns.
 * INPUT FRAMES of a submitted batch must stay valid AND UNCHANGED until its wait returns, whatever memory they live
 * in: frames resident in HBM (on_device) and frames in pinned host memory (ft_host_malloc / hipHostMalloc /
 * hipHostRegister) are read in place by the device after submit has returned; only pageable host frames are copied
 * before submit returns.  A camera ring buffer must therefore not recycle a slot between submit and wait. */
FT_API int ft_stereo_frontend_submit(ft_stereo_frontend *fe, const uint8_t *const *imagesL,
                                     const uint8_t *const *imagesR, int batch, int on_device, int width, int height,
                                     int stride, ft_keypoint *keysL, uint8_t *descL, int *nL, ft_keypoint *keysR,
                                     uint8_t *descR, int *nR, int capacity, float *uright, float *depth,
                                     int *n_matches);
FT_API int ft_stereo_frontend_wait(ft_stereo_frontend *fe);
FT_API int ft_stereo_frontend_process(ft_stereo_frontend *fe, const uint8_t *const *imagesL,
                                      const uint8_t *const *imagesR, int batch, int on_device, int width,
                                      int height, int stride, ft_keypoint *keysL, uint8_t *descL, int *nL,
                                      ft_keypoint *keysR, uint8_t *descR, int *nR, int capacity, float *uright,
                                      float *depth, int *n_matches);
/* the descriptors of pair `slot` of the batch processed last, where the front end left them in HBM (n x 32 bytes in
 * the order of the host results; valid until the front end processes another batch): input of ft_bow_transform
 * (Frame::ComputeBoW) without a copy */
FT_API int ft_stereo_frontend_device_descriptors(ft_stereo_frontend *fe, int slot, int right, const uint8_t **dptr, int *n);

/* ------------------------------------------------------------------------------------------------
 * Fisheye stereo matching (matching part).
 * Replaces KernelController::launchFisheyeStereoMatchKernel(N, Nr, descL, descR, matches)
 * (include/Kernels/KernelController.h:38); semantics follow Frame::ComputeStereoFishEyeMatches
 * (src/Frame.cc:1231-1255): BFMatcher(NORM_HAMMING).knnMatch(k=2) + Lowe ratio 0.7.  The caller passes
 * the lapping-area subsets like the CPU branch (src/Frame.cc:1233-1237).  matches[i] = index into
 * descR or -1; best/second (may be NULL) = the two smallest distances.
 * ---------------------------------------------------------------------------------------------- */
FT_API int ft_fisheye_match(ft_context *ctx, const uint8_t *descL, int nL, const uint8_t *descR, int nR,
                            int *matches, int *best, int *second);

/* Complete Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1231-1271): the 2-NN + ratio test
 * above followed, on the device, by KannalaBrandt8::TriangulateMatches per surviving pair
 * (src/CameraModels/KannalaBrandt8.cpp:306-372: Newton unprojection, parallax, linear triangulation, depth and
 * reprojection tests).  keysL / keysR are the keypoints of the lapping-area subsets descL / descR refer to.
 * matches[i] = index into the right subset or -1 (mvLeftToRightMatch), depth[i] = mvDepth or -1,
 * p3d[3i..3i+2] = mvStereo3Dpoints.  The null vector of the 4x4 triangulation system is computed by a one-sided
 * Jacobi SVD in double (the reference uses Eigen::JacobiSVD in float): depth / p3d agree with the reference to
 * its own rounding error, not bit for bit.  Every other float step is the reference's operation for operation,
 * including tanf / atan2f / cosf / sinf as the host's glibc evaluates them (ft_selftest_libm). */
typedef struct ft_fisheye_rig {
    float cam1[8], cam2[8]; /* fx fy cx cy k1 k2 k3 k4 of mpCamera / mpCamera2 */
    float precision;        /* KannalaBrandt8::precision */
    float Rlr[9], tlr[3];   /* mRlr (row-major), mtlr */
} ft_fisheye_rig;
FT_API int ft_fisheye_stereo(ft_context *ctx, const ft_fisheye_rig *rig, const uint8_t *descL, const ft_keypoint *keysL,
                             int nL, const uint8_t *descR, const ft_keypoint *keysR, int nR, const float *level_sigma2,
                             int nlevels, int *matches, float *depth, float *p3d, int *n_matches);

/* ------------------------------------------------------------------------------------------------
 * Frame view for the projection matchers: the fields of ORB_SLAM3::Frame that
 * DATA_WRAPPER::CudaFrame::setMemory marshals (src/Kernels/CudaWrappers/CudaFrame.cu:77-181).
 * The 64x48 grid (Frame::AssignFeaturesToGrid, src/Frame.cc:409-440) is rebuilt on the device.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_frame_view {
    int N;     /* all keypoints (left + right when Nleft != -1) */
    int Nleft; /* -1: mono / rectified stereo (keys = mvKeysUn); else keys = mvKeys, keys_right = mvKeysRight */
    float mnMinX, mnMinY, mnMaxX, mnMaxY;
    float grid_inv_w, grid_inv_h; /* mfGridElementWidthInv / mfGridElementHeightInv */
    float mbf, mb;
    const ft_keypoint *keys;
    const ft_keypoint *keys_right;
    const uint8_t *descriptors; /* N x 32 (left rows then right rows) */
    const float *uright;        /* mvuRight[N] when Nleft == -1, NULL = all -1 */
    int *holder_obs;            /* in/out [N]: Observations() of mvpMapPoints[i], -1 when NULL */
    const int *left_to_right;   /* mvLeftToRightMatch[Nleft] or NULL */
    const int *right_to_left;   /* mvRightToLeftMatch[N-Nleft] or NULL */
    int cam_model;              /* 0 Pinhole, 1 KannalaBrandt8 */
    float cam[8];               /* fx fy cx cy k1 k2 k3 k4 */
    float Trl[12];              /* row-major 3x4 GetRelativePoseTrl() */
    const float *scale_factors; /* mvScaleFactors[nlevels] */
    int nlevels;
} ft_frame_view;

/* Frame::GetFeaturesInArea (src/Frame.cc:681-747) for nq queries at once, with the 64x48 grid of
 * Frame::AssignFeaturesToGrid / PosInGrid (:409-440, :749-759) evaluated on the device.  Query i = (x[i], y[i], r[i],
 * min_level[i], max_level[i], right[i]) (right may be NULL: left camera).  indices receives, per query, the keypoint
 * indices in the reference's order (cell column, cell row, then insertion order) at indices[i * capacity ...];
 * counts[i] = number of hits; when it exceeds capacity the first `capacity` hits in that order are stored. */
FT_API int ft_features_in_area(ft_context *ctx, const ft_frame_view *F, int nq, const float *x, const float *y,
                               const float *r, const int *min_level, const int *max_level, const uint8_t *right,
                               int *indices, int capacity, int *counts);

/* SoA arrays of the local map points, exactly what SearchLocalPointsKernel::launch builds
 * (src/Kernels/SearchLocalPointsKernel.cu:369-390) plus Observations(). */
typedef struct ft_local_points {
    int M;
    const uint8_t *skip; /* (!mbTrackInView && !mbTrackInViewR) || (bFarPoints && depth > thFar) || isBad() */
    const uint8_t *in_view, *in_view_r;
    const int *level, *level_r;           /* mnTrackScaleLevel, mnTrackScaleLevelR */
    const float *view_cos, *view_cos_r;   /* mTrackViewCos, mTrackViewCosR */
    const float *proj_x, *proj_y;         /* mTrackProjX, mTrackProjY */
    const float *proj_xr, *proj_yr;       /* mTrackProjXR, mTrackProjYR */
    const uint8_t *descriptors;           /* M x 32 */
    const int *observations;              /* pMP->Observations() */
} ft_local_points;

/* Replaces KernelController::launchSearchLocalPointsKernel (include/Kernels/KernelController.h:40-42)
 * AND the acceptance loop around it (src/ORBmatcher.cc:241-308); semantics follow the CPU branch of
 * ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>, th, bFarPoints, thFarPoints)
 * (src/ORBmatcher.cc:49-225) including its in-call claiming order.
 * assign[i] (size F->N) = index of the map point written to F.mvpMapPoints[i], else -1;
 * F->holder_obs is updated like mvpMapPoints.  The ten raw arrays (size M, any may be NULL) are the
 * reference kernel's outputs.  *n_matches = the reference's return value. */
FT_API int ft_search_local_points(ft_context *ctx, ft_frame_view *F, const ft_local_points *P, float th,
                                  float nn_ratio, int *assign, int *n_matches, int *best_dist, int *best_dist2,
                                  int *best_level, int *best_level2, int *best_idx, int *best_dist_r,
                                  int *best_dist2_r, int *best_level_r, int *best_level2_r, int *best_idx_r);

/* Last-frame map points for the motion-model search. */
typedef struct ft_last_points {
    int N;                      /* LastFrame.N */
    const uint8_t *valid;       /* mvpMapPoints[i] != NULL && !mvbOutlier[i] */
    const float *world_pos;     /* N x 3, pMP->GetWorldPos() */
    const uint8_t *descriptors; /* N x 32, pMP->GetDescriptor() */
    const int *observations;
    const int *octave; /* octave of last-frame keypoint i */
    const float *angle; /* angle of last-frame keypoint i (rotation histogram) */
} ft_last_points;

/* Replaces KernelController::launchPoseEstimationKernel (include/Kernels/KernelController.h:44-46) and
 * the histogram loop around it (src/ORBmatcher.cc:2013-2081); semantics follow the CPU branch of
 * ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1775-1990).
 * Tcw: row-major 3x4 current pose; forward/backward as computed at :1794-1795.
 * assign[i] (size Cur->N) = last-frame index whose map point ends up in CurrentFrame.mvpMapPoints[i]. */
FT_API int ft_search_last_frame(ft_context *ctx, ft_frame_view *Cur, const ft_last_points *L, const float *Tcw,
                                float th, int forward, int backward, int check_orientation, int *assign,
                                int *n_matches, int *best_dist, int *best_idx, int *best_dist_r,
                                int *best_idx_r);

/* The same search with the poses in the form the reference's CPU branch multiplies with.  CurrentFrame.GetPose() and
 * GetRelativePoseTrl() are Sophus::SE3f: a unit quaternion and a translation, applied to a point as
 * Thirdparty/Sophus/sophus/so3.hpp:358-367 + se3.hpp:321-324 do (uv = 2 (q.vec x p); p + w uv + q.vec x uv; + t) - NOT as a
 * matrix product; the two differ in the last bits of the projected point, i.e. in whether a keypoint that sits within ~1e-4 px
 * of a search window's edge is a candidate.  ft_search_last_frame (3x4 matrices, y = R x + t) is the form the reference's GPU
 * boundary takes (Eigen::Matrix4f transform_matrix, include/Kernels/KernelController.h:44-46); this one reproduces
 * `Tcw * x3Dw` (src/ORBmatcher.cc:1805) and `GetRelativePoseTrl() * x3Dc` (:1900) of the CPU branch operation for operation.
 * q = Eigen::Quaternionf::coeffs() = (x, y, z, w) of so3().unit_quaternion(); Trl may be NULL when Cur->Nleft == -1 (Cur->Trl is
 * not read by this call). */
typedef struct ft_se3 {
    float q[4];
    float t[3];
} ft_se3;
FT_API int ft_search_last_frame_se3(ft_context *ctx, ft_frame_view *Cur, const ft_last_points *L, const ft_se3 *Tcw,
                                    const ft_se3 *Trl, float th, int forward, int backward, int check_orientation, int *assign,
                                    int *n_matches, int *best_dist, int *best_idx, int *best_dist_r, int *best_idx_r);

/* ------------------------------------------------------------------------------------------------
 * ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/ORBmatcher.cc:747-862), the
 * matcher Tracking::MonocularInitialization calls on every frame until the map exists (src/Tracking.cc:2516-2549:
 * ORBmatcher matcher(0.9, true); windowSize 100).  For the level-0 keypoints of F1 IN INDEX ORDER: the candidates
 * F2.GetFeaturesInArea(prev.x, prev.y, windowSize, 0, 0) in that function's order, a candidate held at a distance that is not
 * larger is skipped (:786), best / second best with strict <, TH_LOW = 50 and bestDist < (float)bestDist2 * nn_ratio (:801-803);
 * a strictly closer keypoint takes the match away from its owner, who stays unmatched (:805-813) but stays in its rotation bin
 * (:817-825); ComputeThreeMaxima and the removal (:831-854), then vbPrevMatched[i1] = F2.mvKeysUn[vnMatches12[i1]].pt (:857-859).
 * Of F1 only N, keys (octave, angle) and descriptors are read; F2 is a mono / rectified view (Nleft == -1): N, keys,
 * descriptors, the image bounds and grid constants, nlevels.  prev_matched: N1 x 2 floats, in/out; matches12: N1 ints
 * (vnMatches12); *n_matches: the return value; matched_distance (may be NULL): F2->N ints, vMatchedDistance as the loop leaves
 * it (INT_MAX where unmatched).  Everything equals the reference bit for bit.
 * Launches per call: 4 (the grid of F2, then three kernels: rows and candidate order, the candidates of every row, the
 * sequential resolution with histogram and outputs) - a fixed sequence, one wait; kernel timing names them kernel.init_*.
 * FT_ERR_CAPACITY when the two frames together hold more than 38400 level-0 keypoints (65534 in F1).
 * ---------------------------------------------------------------------------------------------- */
FT_API int ft_search_for_initialization(ft_context *ctx, const ft_frame_view *F1, const ft_frame_view *F2, float *prev_matched,
                                        int window_size, float nn_ratio, int check_orientation, int *matches12, int *n_matches,
                                        int *matched_distance);

/* ------------------------------------------------------------------------------------------------
 * ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist)
 * (src/ORBmatcher.cc:2087-2208), the matcher Tracking::Relocalization calls behind PnP (src/Tracking.cc:3924: th 10, ORBdist 100;
 * :3938: th 3, ORBdist 64; ORBmatcher matcher2(0.9, true)).  For the keyframe's map points IN INDEX ORDER: x3Dc = Tcw * x3Dw in
 * the Sophus form (see ft_search_last_frame_se3), mpCamera->project, the image bounds - NO depth test: a point behind the camera
 * whose projection lands inside the bounds is searched (:2112-2119) -, dist3D = |x3Dw - Ow| with Ow = Tcw.inverse().translation()
 * (the conjugate of q applied to -t; q is taken as the unit quaternion it is, without the renormalisation of SO3's
 * constructor) against [0.8f min_distance, 1.2f max_distance], PredictScale, radius = th * mvScaleFactors[level], the candidates
 * GetFeaturesInArea(u, v, radius, level - 1, level + 1) of the LEFT camera in that function's order (mvuRight is never looked at).
 * A candidate whose mvpMapPoints entry is not NULL is skipped WHATEVER its Observations(): on entry "held" is holder_obs != -1, and
 * a keypoint written by an earlier point of the call is held for every later one.  Best distance with strict <; bestDist <= ORBdist
 * writes the keypoint; rotation histogram of angle[i] - mvKeysUn[bestIdx2].angle, ComputeThreeMaxima, removal (:2186-2205).
 * Precondition: x3Dc.z != 0 for every valid point (the reference's behaviour is undefined there: NaN into an int cast).
 * assign[i2] (size Cur->N) = the keyframe index whose point ends up in mvpMapPoints[i2], else -1; entries >= Nleft of a
 * two-camera frame are -1.  holder_obs of a keypoint that keeps its write becomes observations[i]; one the histogram removed is
 * -1 again.  best_dist / best_idx (size K->N, may be NULL): bestDist / bestIdx2 as the loop leaves them for point i, 256 / -1 for a
 * point that was skipped or found every candidate held.  *n_matches: the return value.  Everything equals the reference's CPU branch
 * bit for bit (there is no GPU boundary for this function in the reference).
 * Launches per call: 4 (the frame's grid, then three kernels: projection, the candidates of every point, the sequential
 * resolution with histogram and outputs) - a fixed sequence, one wait; kernel timing names them kernel.reloc_*.
 * FT_ERR_CAPACITY, with NO output written and holder_obs unchanged, when the window of one point holds more than 256 free
 * keypoints of its level band, or when 4 bytes per point plus a bit per keypoint exceed 150 KB.  0 <= orb_dist <= 255.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_keyframe_points {
    int N;                      /* pKF->GetMapPointMatches().size() */
    const uint8_t *valid;       /* pMP && !pMP->isBad() && !sAlreadyFound.count(pMP) */
    const float *world_pos;     /* N x 3, GetWorldPos() */
    const float *max_distance;  /* mfMaxDistance (the 1.2f / 0.8f of the invariance getters are applied inside, as in ft_map_points) */
    const float *min_distance;  /* mfMinDistance */
    const uint8_t *descriptors; /* N x 32, GetDescriptor() */
    const int *observations;    /* Observations(): what holder_obs of a written keypoint becomes */
    const float *angle;         /* pKF->mvKeysUn[i].angle; may be NULL when check_orientation == 0 */
} ft_keyframe_points;
FT_API int ft_search_keyframe_projection(ft_context *ctx, ft_frame_view *Cur, const ft_keyframe_points *K, const ft_se3 *Tcw,
                                         float log_scale_factor, float th, int orb_dist, int check_orientation, int *assign,
                                         int *n_matches, int *best_dist, int *best_idx);

/* ------------------------------------------------------------------------------------------------
 * Frustum test + scale prediction for the local map points: Frame::isInFrustum /
 * isInFrustumChecks (src/Frame.cc:536-610, 1308-1382) with MapPoint::PredictScale (src/MapPoint.cc:531-546),
 * the host loop in front of SearchByProjection (src/Tracking.cc:3503-3522).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_frame_pose {
    float Rcw[9]; /* mRcw, row-major */
    float tcw[3]; /* mtcw */
    float Ow[3];  /* mOw */
    float tlr[3]; /* mTlr.translation(), two-camera frames only (Frame.cc:1319) */
} ft_frame_pose;

typedef struct ft_map_points {
    int M;
    const uint8_t *skip;       /* NULL or: mnLastFrameSeen == frame id || isBad() (Tracking.cc:3507-3510) */
    const float *world_pos;    /* M x 3, GetWorldPos() */
    const float *normal;       /* M x 3, GetNormal() */
    const float *max_distance; /* mfMaxDistance (GetMaxDistanceInvariance() is 1.2f times this) */
    const float *min_distance; /* mfMinDistance (GetMinDistanceInvariance() is 0.8f times this) */
    const uint8_t *descriptors; /* M x 32, GetDescriptor()  - read by the searches only */
    const int *observations;    /* Observations()           - read by the searches only */
} ft_map_points;

/* The MapPoint tracking fields isInFrustum writes (arrays of M, each may be NULL): mbTrackInView(R),
 * mnTrackScaleLevel(R), mTrackViewCos(R), mTrackProjX/Y, mTrackProjXR/YR, mTrackDepth(R).  Fields the
 * reference leaves untouched for a point read level -1, view_cos 0, proj -1, depth 0. */
typedef struct ft_frustum_result {
    uint8_t *in_view, *in_view_r;
    int *level, *level_r;
    float *view_cos, *view_cos_r;
    float *proj_x, *proj_y, *proj_xr, *proj_yr;
    float *depth, *depth_r;
} ft_frustum_result;

/* F supplies the frame constants only (Nleft, bounds, camera, Trl, mbf, nlevels); its keypoint arrays are not
 * read.  log_scale_factor = Frame::mfLogScaleFactor.  *n_to_match = number of points in view of a camera. */
FT_API int ft_is_in_frustum(ft_context *ctx, const ft_frame_view *F, const ft_frame_pose *pose, const ft_map_points *P,
                            float viewing_cos_limit, float log_scale_factor, const ft_frustum_result *out,
                            int *n_to_match);

/* ------------------------------------------------------------------------------------------------
 * Device-resident frame for the projection searches.  The reference re-marshals the whole
 * Frame into a CudaFrame on every kernel call (src/Kernels/CudaWrappers/CudaFrame.cu:77-181).  Here the frame
 * is uploaded once (or bound to the buffers a stereo front end already holds in HBM: no copy at all) and is
 * then used by isInFrustum, SearchByProjection(last frame) and SearchByProjection(local map); the occupancy
 * of mvpMapPoints (holder_obs) carries over from one search to the next as in Tracking::TrackWithMotionModel
 * followed by Tracking::SearchLocalPoints, and the frustum outputs feed the local-map search without
 * leaving the device.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_tracked_frame ft_tracked_frame;
FT_API int ft_tracked_frame_create(ft_context *ctx, int max_keypoints, int max_points, ft_tracked_frame **out);
FT_API int ft_tracked_frame_destroy(ft_tracked_frame *tf);
/* copies keys / descriptors / uright / match tables / holder_obs of F to the device and builds its grid.  The arrays of F are
 * read before the call returns (packed into pinned staging of the frame); the device copies and the grid are ordered in front of
 * the searches that follow on the context's stream, the call itself does not wait for them. */
FT_API int ft_tracked_frame_upload(ft_tracked_frame *tf, const ft_frame_view *F);
/* pair `slot` of the batch the front end processed last (rectified stereo, Nleft == -1): keypoints, descriptors
 * and mvuRight are used where ft_stereo_frontend_* left them in HBM.  meta supplies the frame constants and
 * meta->keys (host copy, for the rotation histogram); holder_obs starts at meta->holder_obs or all -1.
 * The binding is valid until the front end processes another batch. */
FT_API int ft_tracked_frame_bind_stereo(ft_tracked_frame *tf, ft_stereo_frontend *fe, int slot, const ft_frame_view *meta);
/* ft_search_last_frame on the resident frame; updates the resident holder_obs */
FT_API int ft_tracked_frame_search_last_frame(ft_tracked_frame *tf, const ft_last_points *L, const float *Tcw, float th,
                                              int forward, int backward, int check_orientation, int *assign,
                                              int *n_matches);
/* the Sophus form of the poses (see ft_search_last_frame_se3) on the resident frame */
FT_API int ft_tracked_frame_search_last_frame_se3(ft_tracked_frame *tf, const ft_last_points *L, const ft_se3 *Tcw,
                                                  const ft_se3 *Trl, float th, int forward, int backward,
                                                  int check_orientation, int *assign, int *n_matches);
/* Tracking::SearchLocalPoints on the resident frame: isInFrustum (viewing_cos_limit, log_scale_factor) for all
 * points, then SearchByProjection(F, points, th, far_points, th_far_points) on the device-resident results.
 * frustum (may be NULL) receives the isInFrustum fields; assign / n_matches as in ft_search_local_points. */
FT_API int ft_tracked_frame_track_local_map(ft_tracked_frame *tf, const ft_frame_pose *pose, const ft_map_points *P,
                                            float viewing_cos_limit, float log_scale_factor, float th, float nn_ratio,
                                            int far_points, float th_far_points, const ft_frustum_result *frustum,
                                            int *n_to_match, int *assign, int *n_matches);
/* ft_search_for_initialization on two resident frames: `initial` (mInitialFrame, uploaded once when it is set) and `current`
 * (uploaded per frame), both by ft_tracked_frame_upload with Nleft == -1 on one context.  Nothing of either frame is marshalled
 * again: prev_matched goes up; matches12, prev_matched and *n_matches come back.  holder_obs of both frames is neither read nor
 * written.  Launches per call: 3 (4 for a current frame loaded under option search_grid = 0: its grid is built for the call);
 * statistic "tracked.search_for_initialization.launches" sums them.  A frame without level-0 keypoints returns without a launch. */
FT_API int ft_tracked_frame_search_for_initialization(ft_tracked_frame *current, ft_tracked_frame *initial, float *prev_matched,
                                                      int window_size, float nn_ratio, int check_orientation, int *matches12,
                                                      int *n_matches);
/* ft_search_keyframe_projection on the resident frame: only K and the pose are marshalled; the frame, its grid and holder_obs
 * stay where ft_tracked_frame_upload / bind_stereo left them, and the resident holder_obs is updated in place, so that a second
 * call (src/Tracking.cc:3938) or ft_tracked_frame_track_local_map sees the writes.  Launches per call: 3 (4 for a frame loaded
 * under option search_grid = 0: its grid is built for the call); statistic "tracked.search_keyframe_projection.launches" sums
 * them.  No point, no valid point or no keypoint returns without a launch. */
FT_API int ft_tracked_frame_search_keyframe_projection(ft_tracked_frame *tf, const ft_keyframe_points *K, const ft_se3 *Tcw,
                                                       float log_scale_factor, float th, int orb_dist, int check_orientation,
                                                       int *assign, int *n_matches);
/* current holder_obs (size N of the resident frame) */
FT_API int ft_tracked_frame_holder_obs(ft_tracked_frame *tf, int *holder_obs);

/* ------------------------------------------------------------------------------------------------
 * B device-resident frames per call ("Batch API (B frames per launch)").  The reference's tracking thread
 * searches one frame at a time (Tracking::TrackWithMotionModel src/Tracking.cc:2911-2989, Tracking::SearchLocalPoints
 * :3472-3555; one kernel launch per call: src/Kernels/SearchLocalPointsKernel.cu:351-435, PoseEstimationKernel.cu:350-371),
 * which leaves a 256-CU device idle by construction.  A batch holds n_frames INDEPENDENT frames - the camera streams of one
 * time step, or any frames whose inputs the caller holds - and runs every stage as ONE launch over all of them: the grid
 * build, isInFrustum, the window scans of a search, and the in-call claiming of all frames (option search_cache = 2, batches of
 * 24 frames and more: one launch, a workgroup per frame walks the frame's points in index order; smaller batches, search_cache
 * <= 1, or a frame with a window of more than 511 candidates: claim passes, one launch per pass for all frames, per-frame
 * convergence).  Per frame the results are those of the
 * ft_tracked_frame_* call on that frame, bit for bit; the holder_obs of every frame carries over from one search to the next.
 * Arrays indexed by frame: frames[], L[], Tcw (12 floats per frame), forward / backward (NULL = all 0), poses[], P[],
 * frustum[] (NULL = not wanted), n_to_match[], assign[] (assign[f] has frames[f].N entries), n_matches[].
 * A batch object has a stream and a lock of its own: calls on one batch are serialised, two batches of one context used from
 * two host threads are two batches in flight.
 * The host's share of a search: the writes of a search (mvpMapPoints[kp] = pMP in point order, the rotation histogram and
 * ComputeThreeMaxima of SearchByProjection(CurrentFrame, LastFrame), src/ORBmatcher.cc:1880-1896, 1966-1987, 2210-2251) are
 * replayed ON THE DEVICE, the frames' holder_obs live in HBM, and the assignments come back through pinned memory - the host
 * builds the job records, enqueues, and copies the assignments into the caller's arrays.  Point arrays (ft_last_points /
 * ft_map_points) that ALL lie in pinned host memory (ft_host_malloc, hipHostMalloc, hipHostRegister) are read in place by the
 * device - no host copy; pageable ones are packed into the batch's pinned staging by the context's host threads first.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_tracked_batch ft_tracked_batch;
FT_API int ft_tracked_batch_create(ft_context *ctx, int max_frames, int max_keypoints, int max_points, ft_tracked_batch **out);
FT_API int ft_tracked_batch_destroy(ft_tracked_batch *tb);
/* ft_tracked_frame_upload for n_frames frames: one packed copy, all grids by one launch */
FT_API int ft_tracked_batch_upload(ft_tracked_batch *tb, int n_frames, const ft_frame_view *frames);
/* The frames of the batch straight from what two extractors left in HBM - no keypoint or descriptor crosses PCIe again.
 * Slot slot0 + f of exL / exR holds the left / right image of two-camera frame f (their last ft_extract_batch calls; lapping areas
 * [lap_l0, lap_l1] / [lap_r0, lap_r1] as passed there).  On the device: keypoints and descriptors are put into the reference's
 * order (lapping-area keypoints filled from the back, src/ORBextractor.cc:1466-1487); Frame::ComputeStereoFishEyeMatches
 * (src/Frame.cc:1231-1271) for every frame - 2-NN + ratio 0.7 between the lapping subsets (the seam of
 * launchFisheyeStereoMatchKernel, include/Kernels/KernelController.h:38) and, when `rig` is given, KannalaBrandt8::
 * TriangulateMatches on every surviving pair (depth > 0.0001 keeps it; level_sigma2 = mvLevelSigma2, nlevels floats) - fills
 * mvLeftToRightMatch / mvRightToLeftMatch; the grids are built.  rig == NULL: the matching alone (every ratio-test survivor stays).
 * meta[f]: the frame constants, N / Nleft (= the counts ft_extract_batch returned), holder_obs or NULL (all -1); its keys /
 * keys_right / descriptors / match tables are not read (the angles of the rotation histogram are read on the device).
 * exL / exR must not be used by another thread during the call; their next batch is ordered behind this call's reads of their slots.
 * Outputs, each an array of n_frames pointers or NULL: left_to_right[f] / right_to_left[f] (the match tables; both or neither),
 * depth[f] / p3d[f] (mvDepth [Nleft], mvStereo3Dpoints [3 Nleft]; with a rig only), n_stereo[f] (the frame's nMatches).  Without
 * outputs the call does not wait for the device. */
FT_API int ft_tracked_batch_bind_fisheye(ft_tracked_batch *tb, ft_extractor *exL, ft_extractor *exR, int slot0, int n_frames,
                                         int lap_l0, int lap_l1, int lap_r0, int lap_r1, const ft_frame_view *meta,
                                         const ft_fisheye_rig *rig, const float *level_sigma2, int *const *left_to_right,
                                         int *const *right_to_left, float *const *depth, float *const *p3d, int *n_stereo);
/* the same with a first slot per camera: exL == exR is allowed - ONE extractor whose last batch holds the left images in slots
 * slot0 .. and the right ones in slots slot0_right .. (disjoint ranges), e.g. a two-camera frame extracted as a batch of two */
FT_API int ft_tracked_batch_bind_fisheye_slots(ft_tracked_batch *tb, ft_extractor *exL, ft_extractor *exR, int slot0, int slot0_right,
                                               int n_frames, int lap_l0, int lap_l1, int lap_r0, int lap_r1,
                                               const ft_frame_view *meta, const ft_fisheye_rig *rig, const float *level_sigma2,
                                               int *const *left_to_right, int *const *right_to_left, float *const *depth,
                                               float *const *p3d, int *n_stereo);
/* ft_tracked_frame_search_last_frame for every frame of the batch (n_frames = the number uploaded) */
FT_API int ft_tracked_batch_search_last_frame(ft_tracked_batch *tb, int n_frames, const ft_last_points *L, const float *Tcw,
                                              float th, const int *forward, const int *backward, int check_orientation,
                                              int *const *assign, int *n_matches);
/* the Sophus form of the poses (ft_search_last_frame_se3); Trl[] may be NULL when no frame has two cameras */
FT_API int ft_tracked_batch_search_last_frame_se3(ft_tracked_batch *tb, int n_frames, const ft_last_points *L, const ft_se3 *Tcw,
                                                  const ft_se3 *Trl, float th, const int *forward, const int *backward,
                                                  int check_orientation, int *const *assign, int *n_matches);
/* ft_tracked_frame_track_local_map for every frame of the batch */
FT_API int ft_tracked_batch_track_local_map(ft_tracked_batch *tb, int n_frames, const ft_frame_pose *poses,
                                            const ft_map_points *P, float viewing_cos_limit, float log_scale_factor, float th,
                                            float nn_ratio, int far_points, float th_far_points,
                                            const ft_frustum_result *frustum, int *n_to_match, int *const *assign,
                                            int *n_matches);
/* The two halves of the three searches above, like ft_stereo_frontend_submit / _wait: submit_* enqueues the search (the claim
 * iteration up to the first point where the host has to look at the device's flag words - the whole search when the one-launch
 * resolution resolves every frame, the usual case) and returns; ft_tracked_batch_wait waits for the device, runs what is left
 * (claim passes for frames the resolution gave up on, small batches), and fills assign / n_matches / n_to_match / frustum.  One
 * search per batch may be in flight: a second submit (or upload / bind_fisheye) before the wait is FT_ERR_INVALID.  Between
 * submit and wait the OUTPUT arrays must stay untouched and point arrays in pinned memory (read in place, see above) must
 * stay valid and UNCHANGED; everything else of the arguments is copied before submit returns.  An input error only the device
 * sees when it reads the arrays in place (a last-frame octave outside the frame's levels) is reported by the wait.
 * ft_tracked_batch_wait without a submitted search returns FT_OK. */
FT_API int ft_tracked_batch_submit_search_last_frame(ft_tracked_batch *tb, int n_frames, const ft_last_points *L, const float *Tcw,
                                                     float th, const int *forward, const int *backward, int check_orientation,
                                                     int *const *assign, int *n_matches);
FT_API int ft_tracked_batch_submit_search_last_frame_se3(ft_tracked_batch *tb, int n_frames, const ft_last_points *L,
                                                         const ft_se3 *Tcw, const ft_se3 *Trl, float th, const int *forward,
                                                         const int *backward, int check_orientation, int *const *assign,
                                                         int *n_matches);
FT_API int ft_tracked_batch_submit_track_local_map(ft_tracked_batch *tb, int n_frames, const ft_frame_pose *poses,
                                                   const ft_map_points *P, float viewing_cos_limit, float log_scale_factor,
                                                   float th, float nn_ratio, int far_points, float th_far_points,
                                                   const ft_frustum_result *frustum, int *n_to_match, int *const *assign,
                                                   int *n_matches);
FT_API int ft_tracked_batch_wait(ft_tracked_batch *tb);
/* current holder_obs of frame `frame` (its N entries): copied down from HBM, where the searches keep it */
FT_API int ft_tracked_batch_holder_obs(ft_tracked_batch *tb, int frame, int *holder_obs);

/* ORBmatcher::DescriptorDistance for n pairs on the device (src/ORBmatcher.cc:2256-2272,
 * device copy src/Kernels/CudaUtils.cu:42-56).  a, b: n x 32 host bytes; dist: n ints. */
FT_API int ft_descriptor_distance(ft_context *ctx, const uint8_t *a, const uint8_t *b, int n, int *dist);

/* Host-libm self test.  The rBRIEF rotation (src/ORBextractor.cc:73-74: std::cos(float), std::sin(float)) and
 * MapPoint::PredictScale (src/MapPoint.cc:539: std::log(float)) are evaluated by the reference with the HOST libm;
 * the kernels reproduce glibc's cosf / sinf / logf bit for bit (fasttrack_amd/csrc/libm_f32.h).  This sweep evaluates
 * func (0 cosf, 1 sinf, 2 logf, 3 atanf, 4 atan2f, 5 tanf) on the device for the float bit patterns first_bits, first_bits + stride,
 * ... <= last_bits and compares with the same function of the calling process's libm.  mismatches == 0 over [0, 0x40c90fdb]
 * (cos, sin) and [1, 0x461c4000] (log, up to 1e4) means the device and this host's libm agree on every argument the path can
 * produce; atanf takes any range up to [0, 0xffffffff]; atan2f(y, x) sweeps y over the range and pairs each y with one x
 * derived from its bits (either sign, 2^-9 <= |x| < 2^7): the KannalaBrandt8 projection of two-camera frames; tanf (its
 * unprojection) is reproduced for |x| < 120, i.e. bits [0, 0x42efffff] and [0x80000000, 0xc2efffff]. */
FT_API int ft_selftest_libm(ft_context *ctx, int func, uint32_t first_bits, uint32_t last_bits, uint32_t stride,
                            unsigned long long *checked, unsigned long long *mismatches, uint32_t *first_bad);

/* ----------------------------------------------------------------------------------------------
 * Frame::ComputeBoW (src/Frame.cc:762-769): DBoW2's
 * TemplatedVocabulary<FORB::TDescriptor, FORB>::transform(features, BowVector&, FeatureVector&, levelsup)
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194) with the tree walk of every descriptor
 * (:1208-1253, FORB::distance Thirdparty/DBoW2/DBoW2/FORB.cpp:81-101) on the device.
 *
 * A vocabulary is the k-ary tree of ORBvoc.txt: node 0 is the root, node i > 0 has parent[i] < i ... (any order of
 * the file is accepted), the children of a node are visited in ascending node id (the order loadFromTextFile
 * appends them, :1369-1420), leaves are the words, numbered in ascending node id.  scoring / weighting use the
 * reference's enum values (BowVector.h:39-56: weighting 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY; scoring 0 L1_NORM,
 * 1 L2_NORM, 2 CHI_SQUARE, 3 KL, 4 BHATTACHARYYA, 5 DOT_PRODUCT).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_vocabulary ft_vocabulary;
/* n_nodes includes the root (entry 0 of every array is ignored except is_leaf); descriptors: n_nodes x 32 bytes */
FT_API int ft_vocabulary_create(ft_context *ctx, int k, int L, int scoring, int weighting, int n_nodes,
                                const int *parent, const uint8_t *is_leaf, const uint8_t *descriptors,
                                const double *weights, ft_vocabulary **out);
/* the text format ORB-SLAM3 ships (TemplatedVocabulary::loadFromTextFile, :1338-1423): "k L scoring weighting", then
 * one line per node: parent is_leaf d0 .. d31 weight */
FT_API int ft_vocabulary_load_text(ft_context *ctx, const char *path, ft_vocabulary **out);
FT_API int ft_vocabulary_destroy(ft_vocabulary *voc);
FT_API int ft_vocabulary_info(const ft_vocabulary *voc, int *k, int *L, int *n_nodes, int *n_words);
/* transform of the n descriptors of one frame (host n x 32 bytes, or a device pointer with on_device != 0, e.g. the
 * descriptors a stereo front end left in HBM).
 * Per feature (each may be NULL): word_ids, node_ids (the ancestor at level L - levelsup, 0 = root if that level is
 * <= 0; the leaf itself if the walk ends above that level), weights (the word's weight; 0 = stopped word).
 * BowVector: bow_ids ascending with bow_values (after the weighting and the normalisation the scoring asks for),
 * n_bow entries (bow_capacity >= n is always enough).
 * FeatureVector in CSR form: fv_nodes ascending, the feature indices of node j (ascending, as push_back leaves them)
 * are fv_features[fv_offsets[j] .. fv_offsets[j + 1]), n_fv nodes (fv_nodes / fv_offsets hold fv_capacity and
 * fv_capacity + 1 entries, fv_features n). */
FT_API int ft_bow_transform(ft_vocabulary *voc, const uint8_t *descriptors, int n, int on_device, int levelsup,
                            unsigned *word_ids, unsigned *node_ids, double *weights, unsigned *bow_ids,
                            double *bow_values, int bow_capacity, int *n_bow, unsigned *fv_nodes, int *fv_offsets,
                            unsigned *fv_features, int fv_capacity, int *n_fv);

/* ----------------------------------------------------------------------------------------------
 * ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, std::vector<MapPoint*> &vpMapPointMatches)
 * (src/ORBmatcher.cc:322-524; Tracking::TrackReferenceKeyFrame src/Tracking.cc:2732-2744 and Relocalization): the step
 * that consumes the FeatureVectors of ft_bow_transform.  A side is its FeatureVector in that CSR form, its descriptors and,
 * for the rotation-consistency filter (mbCheckOrientation), its keypoint angles.  kf_has_point[i] != 0 <=> the keyframe's
 * i-th map point exists and is not bad (:345-351).  frame_nleft = Frame::Nleft (-1 = one camera; otherwise descriptors and
 * angles of the right camera follow the left ones, :383-421 incl. the disabled ratio test of the right camera, :453).
 * matches[i] (i < frame->n) = index of the keyframe feature whose map point vpMapPointMatches[i] receives, or -1;
 * *n_matches = the function's return value.  TH_LOW = 50, HISTO_LENGTH = 30 as in the reference (:42-43). */
typedef struct ft_bow_side {
    int n;                       /* features (descriptors, angles) */
    int n_nodes;                 /* FeatureVector entries */
    const unsigned *fv_nodes;    /* [n_nodes] ascending */
    const int *fv_offsets;       /* [n_nodes + 1] */
    const unsigned *fv_features; /* [fv_offsets[n_nodes]] */
    const uint8_t *descriptors;  /* n x 32 bytes, host */
    const float *angles;         /* [n] cv::KeyPoint::angle; may be NULL without check_orientation */
} ft_bow_side;
FT_API int ft_search_by_bow(ft_context *ctx, const ft_bow_side *kf, const uint8_t *kf_has_point, const ft_bow_side *frame,
                            int frame_nleft, float nn_ratio, int check_orientation, int *matches, int *n_matches);
/* The same search for one frame against ALL the candidate keyframes of a call: the loop of Tracking::Relocalization
 * (src/Tracking.cc:3839-3860; the candidates' isBad() test stays with the caller), whose calls share the frame and are
 * independent of each other.  matches[k * frame->n + i] = the feature index of keyframe k whose map point
 * vvpMapPointMatches[k][i] receives, or -1; n_matches[k] = the return value of the reference's call for candidate k.  Row k is bit
 * for bit what ft_search_by_bow(ctx, &keyframes[k].side, keyframes[k].has_point, frame, frame_nleft, ...) delivers: <= TH_LOW
 * (50 is accepted), the ratio as one fp32 product with a strict <, the first of the node's list at the smallest distance, the
 * frame features an earlier keyframe feature of the node has claimed skipped, the right camera's second best pair with its ratio
 * test disabled (:458), then the rotation histogram of kf angle - frame angle, ComputeThreeMaxima and the removal.  A claim of one
 * candidate is never visible to another.
 * frame_descriptors_on_device != 0: frame->descriptors is a device pointer (ft_stereo_frontend_device_descriptors,
 * ft_device_malloc memory, ...); the descriptors are read in place and never copied.  They must be complete before the call:
 * written by work on the context's own stream, or by work the caller has waited for (as for ft_bow_transform's on_device).
 * Launches per call: 2 whatever n_keyframes (the walk of every (candidate, node) unit; histogram, removal and counts, a workgroup
 * per candidate), one copy up, one copy down, one wait; kernel timing names them kernel.bow_cand_match / kernel.bow_cand_finish.
 * Stats: search_by_bow_candidates.total (ms), .launches, and .up_bytes (the bytes of the copy up, summed in the stat's value).
 * frame->n == 0 or n_keyframes == 0 returns without a launch, n_matches all 0.  A candidate with n == 0, without nodes, without map
 * points or without a shared node gives a row of -1 and 0.
 * FT_ERR_INVALID: what ft_search_by_bow rejects in a side, on any side; frame_nleft outside [-1, frame->n]; null has_point with
 * n > 0; check_orientation without angles on a non-empty side; a frame feature listed twice in the frame's FeatureVector (the
 * independence of the nodes rests on a frame feature sitting in one node); n_keyframes outside [0, 65535]; null matches /
 * n_matches when there is something to write.  FT_ERR_CAPACITY when one call's block exceeds 4 GB.  Nothing is written on an error. */
typedef struct ft_bow_candidate {
    ft_bow_side side;          /* KeyFrame::N, mFeatVec as CSR, mDescriptors, angles[n] (right camera behind the left one, as for ft_search_by_bow) */
    const uint8_t *has_point;  /* [side.n]  GetMapPoint(i) != NULL && !isBad()  (src/ORBmatcher.cc:354-360) */
} ft_bow_candidate;
FT_API int ft_search_by_bow_candidates(ft_context *ctx, const ft_bow_side *frame, int frame_nleft,
                                       int frame_descriptors_on_device,
                                       int n_keyframes, const ft_bow_candidate *keyframes /* [n_keyframes] */,
                                       float nn_ratio, int check_orientation,
                                       int *matches /* n_keyframes x frame->n */, int *n_matches /* [n_keyframes] */);

/* ----------------------------------------------------------------------------------------------
 * ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint*> &vpMatches12) (src/ORBmatcher.cc:864-1004),
 * the first step of LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:657-668), for keyframe 1 against ALL the
 * keyframes of a call: the calls of the reference's loop share keyframe 1 and are independent of each other.
 * For every vocabulary node the two FeatureVectors share, keyframe 1's features are taken in the order of the node's list.  A
 * feature idx1 is skipped when n_left != -1 && idx1 >= n_un (:899: mvKeysUn of a two-camera keyframe holds the left keypoints
 * only, so a FeatureVector may list right-camera features and they are skipped) or when has_point[idx1] == 0 (no map point, or
 * a bad one, :903-907).  A candidate idx2 of the same node in keyframe 2 is skipped under the same two conditions (:919,
 * :925-929) and when an earlier feature of keyframe 1 has taken it (vbMatched2); a skipped candidate is neither best nor second
 * best.  bestDist1 / bestIdx2 / bestDist2 follow a strict < in scan order (:935-944): the best candidate is the first of the
 * node's list with the smallest distance, bestDist2 stays 256 with one candidate.  Accepted when bestDist1 < TH_LOW - strictly:
 * 50 is rejected (:947; the KeyFrame, Frame overload above has <=) - and (float)bestDist1 < nn_ratio * (float)bestDist2, one
 * fp32 product.  Then the rotation histogram of angle1[idx1] - angle2[bestIdx2], ComputeThreeMaxima and the removal (:954-964,
 * :983-1001).
 * matches12[k * kf1->side.n + idx1] = the feature index idx2 of keyframe k whose map point vpMatches12[idx1] receives, or -1;
 * n_matches[k] = the return value.  n_keyframes == 1 is the reference's single call; a keyframe 2 with n == 0, without map
 * points or without a shared node gives all -1 and 0.
 * Launches per call: 2 whatever n_keyframes (the walk of every (node, keyframe 2) pair; histogram, removal and counts, a
 * workgroup per keyframe 2), one copy up, one copy down, one wait; kernel timing names them kernel.bow_kf_match /
 * kernel.bow_kf_finish.  kf1->side.n == 0 or n_keyframes == 0 returns without a launch.
 * FT_ERR_INVALID: what ft_search_by_bow rejects in a side (fv_nodes not strictly ascending, an fv_features entry >= n, null
 * arrays); an fv_features entry listed twice; n_left outside [-1, n]; n_un outside [0, n] when n_left != -1; check_orientation
 * without angles; null has_point.  n < 2^20 per keyframe; FT_ERR_CAPACITY when one call's keyframes exceed 4 GB.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_bow_keyframe {
    ft_bow_side side;          /* n = KeyFrame::N, mFeatVec as CSR, mDescriptors, angles[n] (cv::KeyPoint::angle of mvKeysUn; entries >= n_un are not read) */
    const uint8_t *has_point;  /* [n] GetMapPoint(i) != NULL && !isBad() */
    int n_left;                /* KeyFrame::NLeft, -1 = one camera */
    int n_un;                  /* mvKeysUn.size(); read only when n_left != -1 */
} ft_bow_keyframe;
FT_API int ft_search_by_bow_keyframes(ft_context *ctx, const ft_bow_keyframe *kf1, int n_keyframes,
                                      const ft_bow_keyframe *kf2 /* [n_keyframes] */, float nn_ratio, int check_orientation,
                                      int *matches12 /* n_keyframes x kf1->side.n */, int *n_matches /* [n_keyframes] */);

/* ----------------------------------------------------------------------------------------------
 * ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, vMatchedPairs, bOnlyStereo, bCoarse)
 * (src/ORBmatcher.cc:1006-1245), the matcher of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:388-466), for keyframe 1
 * against ALL the neighbours that passed the caller's baseline filter in one call: the calls of the reference's neighbour loop
 * share keyframe 1 and are independent of each other.
 * For every vocabulary node the two FeatureVectors share and every feature idx1 of keyframe 1 in it: skipped when it has a map
 * point (has_point: the pointer alone, not isBad(), :1073) or when only_stereo && !bStereo1 (bStereo1 = !two_cameras &&
 * uright[idx1] >= 0, :1078).  A candidate idx2 of the same node in keyframe 2 is eligible when it has no map point, is stereo if
 * only_stereo, DescriptorDistance <= TH_LOW (50), is not near the epipole (only when neither feature is stereo and the keyframes
 * have one camera: rejected when distex^2 + distey^2 < 100 * scale_factors2[kp2.octave], strictly, :1125-1133) and, unless
 * coarse, passes pCamera1->epipolarConstrain (:1171).  The match is the eligible candidate of smallest distance, among equals the
 * LAST of the node's list (the scan skips on dist > bestDist, :1116; vbMatched2 is never written, :1048, so no feature sees what
 * another one chose).  Then the rotation histogram of kp1.angle - kp2.angle, ComputeThreeMaxima and the removal (:1186-1232).
 * Keypoints: mvKeysUn when n_left == -1, else mvKeys followed by mvKeysRight (bRight = idx >= n_left).
 * The constraint, float without contraction: pinhole (src/CameraModels/Pinhole.cpp:107-129) a = (x1 F(0,0) + y1 F(1,0)) + F(2,0),
 * b, c likewise, num = (a x2 + b y2) + c, den = a a + b b, false when den == 0, else (double)(num num / den) < 3.84 *
 * (double)level_sigma2_2[kp2.octave]; KannalaBrandt8 (src/CameraModels/KannalaBrandt8.cpp:216-220) TriangulateMatches(...) >
 * 0.0001f as in ft_fisheye_stereo, for two-camera keyframes with the cameras and the pose of the pairing ll, lr, rl, rr of the
 * two features (:1135-1169).  The constants of a pair are Sophus / Eigen expressions on the poses (:1013-1042) and stay with the
 * caller (ft_triang_pair; INTEGRATION.md has the lines).
 * matches12[k * kf1->n + idx1] = vMatches12[idx1] against neighbour k (vMatchedPairs = the entries >= 0 in ascending idx1),
 * n_matches[k] = the return value, best_dist (same shape, may be NULL) = bestDist as the loop leaves it: 50 where nothing was
 * eligible or the feature was skipped.  Everything equals the reference's CPU text bit for bit (the null vector of
 * TriangulateMatches as documented at ft_fisheye_stereo).  n_neighbours == 1 is the reference's single call; a neighbour with
 * n == 0 or without a shared node gives all -1 and 0.
 * Launches per call: 2 whatever n_neighbours (the candidates of every feature against every neighbour; histogram, removal and
 * counts, a workgroup per neighbour), one copy up, one copy down, one wait; kernel timing names them kernel.triang_match /
 * kernel.triang_finish.  kf1->n == 0 or n_neighbours == 0 returns without a launch.
 * FT_ERR_INVALID: a pinhole keyframe with two_cameras; keyframes of one call that differ in two_cameras or in cam_model (the
 * reference reads an uninitialised R12 there); an fv_features entry >= n or listed twice; a keypoint octave outside
 * [0, nlevels); fv_nodes not strictly ascending.  n < 2^20 per keyframe; FT_ERR_CAPACITY when one call's keyframes exceed 4 GB.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_triang_keyframe {
    int n;                       /* KeyFrame::N */
    int n_left;                  /* KeyFrame::NLeft (-1: one camera) */
    const ft_keypoint *keys;     /* [n] mvKeysUn, or mvKeys then mvKeysRight: pt, octave, angle are read */
    const uint8_t *descriptors;  /* n x 32, mDescriptors */
    int n_nodes;                 /* mFeatVec in the CSR form of ft_bow_transform / ft_bow_side */
    const unsigned *fv_nodes;    /* [n_nodes] ascending */
    const int *fv_offsets;       /* [n_nodes + 1] */
    const unsigned *fv_features; /* [fv_offsets[n_nodes]] */
    const uint8_t *has_point;    /* [n] GetMapPoint(i) != NULL */
    const float *uright;         /* [n] mvuRight, or NULL: all -1 */
    int two_cameras;             /* mpCamera2 != NULL */
    int cam_model;               /* 0 pinhole, 1 KannalaBrandt8 */
    float cam[8], cam2[8];       /* fx fy cx cy k1 k2 k3 k4 of mpCamera / mpCamera2 (KannalaBrandt8 only) */
    const float *scale_factors;  /* [nlevels] mvScaleFactors */
    const float *level_sigma2;   /* [nlevels] mvLevelSigma2 */
    int nlevels;
} ft_triang_keyframe;
typedef struct ft_triang_pair {
    float ep[2];         /* pKF2->mpCamera->project(T2w * pKF1->GetCameraCenter()) (:1016-1019) */
    float F12[9];        /* pinhole: K1.transpose().inverse() * hat(t12) * R12 * K2.inverse(), row-major */
    float R12[4][9];     /* KannalaBrandt8: rotationMatrix() (row-major) of T12 (one camera) or Tll; then of Tlr, Trl, Trr */
    float t12[4][3];     /* translation() of the same */
    float kb8_precision; /* KannalaBrandt8::precision */
} ft_triang_pair;
FT_API int ft_search_for_triangulation(ft_context *ctx, const ft_triang_keyframe *kf1, int n_neighbours,
                                       const ft_triang_keyframe *kf2 /* [n_neighbours] */, const ft_triang_pair *pairs /* [n_neighbours] */,
                                       int only_stereo, int coarse, int check_orientation, int *matches12 /* n_neighbours x kf1->n */,
                                       int *n_matches /* [n_neighbours] */, int *best_dist /* may be NULL */);

/* ----------------------------------------------------------------------------------------------
 * The triangulation of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:483-692): what the reference does with every pair
 * of vMatchedPairs behind SearchForTriangulation, here for every match of keyframe 1 against ALL its neighbours in one launch,
 * either on host match rows (ft_triangulate_new_points) or on the rows the matcher left on the device
 * (ft_search_and_triangulate: the matches neither come down nor go up in between).
 * Per match (idx1, idx2) of neighbour k, operation for operation, float without contraction:
 *   keypoints, bRight, bStereo as in ft_search_for_triangulation (bStereo = !two_cameras && uright[idx] >= 0, :492, :501); two-camera
 *   keyframes take pose, camera centre and camera of the pairing ll / lr / rl / rr per match (:505-555).
 *   xn = pCamera->unprojectEig(kp.pt) (Pinhole.cpp:61-64 with cam[]; KannalaBrandt8.cpp:111-143 with kb8_precision), ray = Rwc *
 *   xn with Rwc = Rcw.transpose() (a three-term sum is e0 + (e1 + e2)), cosParallaxRays = ray1.dot(ray2) / (ray1.norm() *
 *   ray2.norm()) (:558-563).  cosParallaxStereo1 = cosf(2 * atan2f(mb1 / 2, depth1[idx1])) when bStereo1, ELSE IF bStereo2
 *   cosParallaxStereo2 likewise, each cosParallaxRays + 1 otherwise; cosParallaxStereo = std::min of the two (:565-576).  The
 *   float overloads bind: LocalMapping.cc sees `using namespace std` through LocalMapping.h -> KeyFrame.h -> ORBVocabulary.h ->
 *   DBoW2/TemplatedVocabulary.h:36.
 *   The branch (:582-604): cosParallaxRays < cosParallaxStereo && > 0 && (bStereo1 || bStereo2 || (double) < 0.9996 (inertial) /
 *   0.9998 (not inertial)): GeometricTools::Triangulate (src/GeometricTools.cc:47-66; rows xn(0) * T.row(2) - T.row(0), ... in
 *   float, false when the fourth component of the null vector == 0, else head(3) / w); else bStereo1 && cosParallaxStereo1 <
 *   cosParallaxStereo2: KeyFrame::UnprojectStereo of keyframe 1 (src/KeyFrame.cc:755-772: keys_raw, x = (u - cx) * z * invfx,
 *   x3D = Rwc * x3Dc + twc, false when depth <= 0); else the same for keyframe 2; else the pair is dropped.
 *   z = Rcw.row(2).dot(x3D) + tcw(2) > 0 in both keyframes; the reprojection tests (:621-672): non-stereo pCamera->project(x, y, z)
 *   against kp.pt with (double)(ex^2 + ey^2) > 5.991 * sigma2, stereo u = fx * x * invz + cx (invz = (float)(1.0 / z)), u_r = u -
 *   mbf * invz with > 7.8 * sigma2 - keyframe 2's u_r with KEYFRAME 1's mbf, as the reference's :665 has it; scale consistency
 *   (:675-691): dist = (x3D - Ow).norm(), zero distances, far_points && (dist >= th_far_points), ratioDist = dist2 / dist1 against
 *   scale_factors1[kp1.octave] / scale_factors2[kp2.octave] and ratio_factor (1.5f * mfScaleFactor).  A NaN passes or fails where the
 *   C++ comparisons let it.
 * Outputs, in the shape of matches12: status[k * kf1->n + idx1] =
 *    0 no match            1 accepted, triangulated     2 accepted, stereo point of keyframe 1     3 ... of keyframe 2
 *   -1 low parallax and no stereo (:603)   -2 Triangulate / UnprojectStereo returned false   -3 z1 <= 0   -4 z2 <= 0
 *   -5 / -6 reprojection error in keyframe 1 / 2     -7 zero distance     -8 far point     -9 scale inconsistency
 * x3d[3 * (k * kf1->n + idx1)]: the point where status > 0, zeros elsewhere; n_points[k]: the accepted points of neighbour k;
 * first_neighbour[idx1]: the smallest k with status > 0, -1 = none.
 * LOOP ORDER.  The reference attaches the new point to idx1 at the first neighbour that accepts it, and its matcher then skips
 * idx1 for the later neighbours (pMP1, src/ORBmatcher.cc:1073).  The batched calls treat the neighbours independently: a later
 * neighbour may report a match and a point for an idx1 that an earlier one took.  first_neighbour[idx1] says which neighbour
 * wins: the caller attaches only the point of that neighbour.  This is not the reference's loop in one respect: there the
 * features taken by earlier neighbours are missing from a later neighbour's rotation histogram (:1186-1232), here they are in
 * it, so with check_orientation the three kept bins of a later neighbour can differ.  n_neighbours == 1 with has_point updated
 * between the calls is the reference's loop exactly.
 * NOT pinned bit for bit: the null vector is a one-sided Jacobi SVD in double, narrowed to float, where the reference runs Eigen's
 * float JacobiSVD (as documented at ft_fisheye_stereo); x3d of triangulated points, and the status of pairs that sit on a
 * threshold, agree with the reference to its rounding error.  Stereo points (status 2, 3) and everything in front of the SVD are
 * the reference's floats.
 * ft_triangulate_new_points: one copy up, ONE launch (kernel.triang_points: a workgroup per neighbour and 256 slots of its row,
 * the slots that hold a match compacted in front of the arithmetic), one copy down, one wait; the fv_*, descriptors and has_point
 * fields of the keyframes are not read and may be NULL.  ft_search_and_triangulate: the arguments and results of
 * ft_search_for_triangulation plus the above in one arena: one copy up, 3 launches, one copy down, one wait, whatever
 * n_neighbours.  kf1->n == 0 or n_neighbours == 0 returns without a launch (counts 0).
 * FT_ERR_INVALID: what ft_search_for_triangulation rejects of the fields that are read; a matches12 entry >= kf2[k].n; a keypoint
 * with uright >= 0 in a keyframe with one camera and depth == NULL; keyframes that differ in two_cameras or cam_model.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_newpoint_geometry {   /* one per keyframe */
    float Tcw[12], Ow[3];               /* GetPose().matrix3x4() row-major, GetCameraCenter() */
    float Tcw_right[12], Ow_right[3];   /* GetRightPose(), GetRightCameraCenter(); read when two_cameras */
    float Rwc[9], twc[3];               /* mRwc, mTwc.translation(): KeyFrame::UnprojectStereo (NOT Rcw^T: taken as given) */
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
    const float *depth;                 /* [n] mvDepth, NULL: no stereo keypoints */
    const ft_keypoint *keys_raw;        /* [n] mvKeys for UnprojectStereo, NULL: same as keys */
    float kb8_precision;                /* KannalaBrandt8::precision of the keyframe's cameras (unprojectEig); unread for pinhole */
} ft_newpoint_geometry;
FT_API int ft_triangulate_new_points(ft_context *ctx, const ft_triang_keyframe *kf1, const ft_newpoint_geometry *g1, int n_neighbours,
                                     const ft_triang_keyframe *kf2 /* [n_neighbours] */, const ft_newpoint_geometry *g2 /* [n_neighbours] */,
                                     const int *matches12 /* n_neighbours x kf1->n, -1 = no match */, int inertial, int far_points,
                                     float th_far_points, float ratio_factor, int *status /* n_neighbours x kf1->n */,
                                     float *x3d /* n_neighbours x kf1->n x 3 */, int *n_points /* [n_neighbours] */,
                                     int *first_neighbour /* [kf1->n] */);
FT_API int ft_search_and_triangulate(ft_context *ctx, const ft_triang_keyframe *kf1, const ft_newpoint_geometry *g1, int n_neighbours,
                                     const ft_triang_keyframe *kf2 /* [n_neighbours] */, const ft_newpoint_geometry *g2 /* [n_neighbours] */,
                                     const ft_triang_pair *pairs /* [n_neighbours] */, int only_stereo, int coarse, int check_orientation,
                                     int inertial, int far_points, float th_far_points, float ratio_factor,
                                     int *matches12 /* n_neighbours x kf1->n */, int *n_matches /* [n_neighbours] */,
                                     int *best_dist /* may be NULL */, int *status, float *x3d, int *n_points, int *first_neighbour);

/* ------------------------------------------------------------------------------------------------
 * Optimizer::PoseOptimization(Frame *pFrame) (src/Optimizer.cc:814-1114): motion-only bundle adjustment, the solver the tracking
 * thread runs behind SearchByProjection(Cur, Last) (src/Tracking.cc:2989), SearchByBoW (TrackReferenceKeyFrame), SearchLocalPoints
 * (:3080) and up to three times per candidate in Relocalization.  n_frames INDEPENDENT frames per call, all of them in ONE launch
 * (a workgroup per frame): the four rounds, g2o's Levenberg-Marquardt inside each (at most 10 iterations of at most 10 trials),
 * the outlier classification between the rounds.  No host round trip inside, no CPU path.
 *
 * The call reproduces, per frame: the edges in keypoint-index order (:858-993) - a mono edge where uright < 0 (or uright == NULL),
 * a stereo edge otherwise; with two cameras (Nleft != -1) a left edge for i < Nleft and a to-body edge of the right camera behind
 * it; nInitialCorrespondences < 3 returns 0 and leaves the pose (mvbOutlier of the correspondences is cleared: the reference
 * clears it while it builds the edges, in front of that return); errors, Jacobians, the quadratic form with the Huber kernel
 * (float delta, float dsqr), computeLambdaInit, the rho / _ni / _nBad bookkeeping, SE3Quat::exp with its small-angle branch; every
 * round restarts from the INPUT pose; an outlier's error is recomputed at the final estimate while an inlier's chi2 is what the
 * last evaluated estimate left (the rejected one when the run ended on a rejected trial); float thresholds 5.991 / 7.815 against a
 * float chi2; the robust kernel dropped behind the classification of round 2; the `< 10` break on ALL edges.  All arithmetic in
 * double, the sums over the edges sequential in keypoint order (g2o's order).  The outlier sweep behind the call
 * (Tracking.cc:2992-3020) stays with the caller.  Not the reference's: the 6 x 6 LDLT does not pivot (a factor that is not > 0
 * makes the trial's chi2 DBL_MAX), and sin / cos / atan2 of doubles are fdlibm's kernels (<= 1 ulp off glibc's); DESIGN.md section 4.
 *
 * Outputs per frame: Tcw_out[f], the float pose of :1109-1111 (w >= 0); outlier[f][i] = mvbOutlier[i] for the i with has_point,
 * untouched elsewhere; n_inliers[f] = nInitialCorrespondences - nBad; trace[f] (NULL: none) per round the iterations optimize()
 * ran, the rejected trials and the last currentChi (0 for a round that did not run).
 * FT_ERR_INVALID: null arrays, N outside [0, 2^24), Nleft outside -1 / [0, N], nlevels outside [1, 12], an unknown camera model,
 * the octave of a correspondence outside [0, nlevels), Tcw.q (Trl.q with two cameras) not a unit quaternion, n_frames < 0.
 * FT_ERR_CAPACITY: a frame with more than FT_POSE_OPT_MAX_EDGES correspondences.  Nothing is written on an error.
 * ---------------------------------------------------------------------------------------------- */
#define FT_POSE_OPT_MAX_EDGES 2000
typedef struct ft_pose_opt_frame {
    int N;                          /* Frame::N */
    int Nleft;                      /* Frame::Nleft, -1 = !mpCamera2 */
    const uint8_t *has_point;       /* [N] mvpMapPoints[i] != NULL */
    const float *world_pos;         /* N x 3 GetWorldPos(); read where has_point */
    const ft_keypoint *keys;        /* Nleft == -1: mvKeysUn [N]; else mvKeys [Nleft].  pt and octave are read */
    const ft_keypoint *keys_right;  /* mvKeysRight [N - Nleft]; read when Nleft != -1 */
    const float *uright;            /* [N] mvuRight, or NULL: no stereo keypoints; read when Nleft == -1 */
    const float *inv_level_sigma2;  /* [nlevels] mvInvLevelSigma2 */
    int nlevels;
    int cam_model;                  /* 0 Pinhole, 1 KannalaBrandt8: mpCamera and mpCamera2 */
    float cam[8], cam2[8];          /* their parameters; a stereo edge reads cam[0..3] as fx, fy, cx, cy */
    float mbf;
    ft_se3 Tcw;                     /* GetPose() */
    ft_se3 Trl;                     /* GetRelativePoseTrl(); read when Nleft != -1 */
} ft_pose_opt_frame;
typedef struct ft_pose_opt_trace {
    int iterations[4], rejected[4];
    double chi2[4];
} ft_pose_opt_trace;
FT_API int ft_pose_optimization(ft_context *ctx, int n_frames, const ft_pose_opt_frame *frames /* [n_frames] */,
                                ft_se3 *Tcw_out /* [n_frames] */, uint8_t *const *outlier /* [n_frames] of [N] */,
                                int *n_inliers /* [n_frames] */, ft_pose_opt_trace *trace /* [n_frames] or NULL */);

/* ------------------------------------------------------------------------------------------------
 * Sim3Solver (src/Sim3Solver.cc): the RANSAC over Horn's closed-form Sim3 that LoopClosing::DetectCommonRegionsFromBoW runs per
 * candidate between SearchByBoW (ft_search_by_bow_keyframes) and SearchByProjection(KeyFrame, Sim3) (ft_search_keyframe_sim3)
 * (src/LoopClosing.cc:698-710).  n_problems INDEPENDENT solvers per call - the loop and merge candidates of a keyframe - and all
 * hypotheses of all of them in THREE launches whatever n_problems is (kernel.sim3_hypotheses: a lane per (problem, iteration);
 * kernel.sim3_count: a wave per (problem, iteration); kernel.sim3_select: a workgroup per problem), one copy up, one copy down,
 * one wait; statistics sim3_solver.total, sim3_solver.launches.  No CPU path.
 *
 * One problem is one Sim3Solver object driven as its only call site drives it: SetRansacParameters(probability, min_inliers,
 * max_iterations) (:123-147), then iterate(20, ...) (:218-294) until bConverge || bNoMore - the solver's state persists between
 * the chunks of 20, so the chunking has no effect; find() (:296-300) is the same loop.
 * The constructor (:35-121): of the n = mN1 entries of vpMatched12 those with valid[i] != 0 survived the pointer, isBad() and
 * index tests of :73-91 (the caller's, on its map) and form the N pairs, in index order: mvX3Dc1 / mvX3Dc2 = Rcw * X + tcw of
 * world_pos1 / world_pos2 (float; Rcw the rotation matrix of Tcw.q; a three-term sum is e0 + (e1 + e2)), mvnMaxError1 / 2 =
 * 9.210 * sigma2 (a double product rounded to float), mvP1im1 / mvP2im2 = pCamera->project of the camera-frame points (made on the
 * host with the device's text), mvnIndices1.  sigma2_1 / sigma2_2 are mvLevelSigma2[kp.octave] of each side PER PAIR: the constructor
 * reads the second through pKFm (as written, :40-45 and :84-85, pKFm is pKF2 for every pair - bDifferentKFs is set only when the
 * vector was empty; the interface does not depend on that).  The two cameras may be of different models.
 * SetRansacParameters: epsilon = (float)min_inliers / N; nIterations = ceil(log(1 - probability) / log(1 - pow(epsilon, 3))) in
 * double, 1 when min_inliers == N; mRansacMaxIts = max(1, min(nIterations, max_iterations)) - result.effective_iterations.
 * NOT the reference's: the min is taken in DOUBLE, an infinite or NaN quotient counting as more than max_iterations (the
 * reference converts the double to int first, which is undefined for a small epsilon).
 * An iteration (:245-263): three draws pick three distinct pairs - rand_draws holds raw rand() values, three per iteration in the
 * reference's order; each is reduced as DUtils::Random::RandomInt does, int((double)r / (RAND_MAX + 1.0) * d), d = N, N - 1, N - 2,
 * against a fresh copy of mvAllIndices with the swap-with-back removal of :177-185.  NOT the reference's: every one of the
 * effective iterations is evaluated and consumes its three draws (the first 3 * effective_iterations entries are read, all
 * 3 * max_iterations are checked), where the reference stops drawing when it converges.
 * ComputeSim3 (:311-414): every float step in the reference's order without contraction - centroids (rowwise().sum() / 3), M =
 * Pr2 * Pr1^T, the ten N entries as float sums, ang = atan2f(|vec|, q0), vec = 2 ang vec / |vec| unless |vec| == 0,
 * Sophus::SO3f::exp with its small-angle branch (theta^2 < 1e-5f * 1e-5f), sinf / cosf / atan2f as glibc evaluates them, the
 * quaternion's matrix, P3 = R * Pr2, ms12i = (float)((double)nom / (double)den) or 1.0f with fix_scale, mt12i = O1 - (s R) O2,
 * mT12i, mT21i with sRinv = (float)(1.0 / s) * R^T and tinv = (-sRinv) * t.  NOT the reference's, each to its rounding error:
 *   the eigenvector of N's largest eigenvalue is Eigen::EigenSolver<Matrix4f>'s in the reference (a real-Schur solver run on a
 *   symmetric matrix); here a cyclic two-sided Jacobi in DOUBLE on the float N: pivots (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) per
 *   sweep, a pivot rotated away unless it is 0 or at most 1e-18 (|app| + |aqq|), until a sweep rotates nothing or 30 sweeps; the
 *   largest diagonal entry, the first on a tie; the sign normalised to q0 >= 0 (the rotation does not depend on it; ang and the
 *   bits do); narrowed to float.  For a degenerate sample (a repeated largest eigenvalue: collinear or coincident points)
 *   agreement with Eigen is not defined;
 *   nom and den, sums of nine float products, are added one after the other in column-major order (Eigen's reduction order of a
 *   3 x 3 array is not pinned).
 * A NaN or infinite scale (den == 0: three coincident points) makes every error NaN, err < max false and the count 0.
 * CheckInliers (:417-441): per pair P3Dc = R X + t of mT12i on mvX3Dc2 through camera 1 and of mT21i on mvX3Dc1 through camera
 * 2 (neither projection tests the depth), the squared distances to mvP1im1 / mvP2im2, inlier when err1 < max1 && err2 < max2.
 * The selection of iterate, evaluated on the counts: the run stops at the first iteration whose count is > min_inliers (an
 * earlier, larger count would have stopped it), else after effective_iterations; mBest* is the LAST iteration up to the stop
 * whose count equals the largest of that prefix (the test at :265 is >=).
 *
 * result[p]: converged = bConverge, no_more = bNoMore, iterations = mnIterations at exit, n_inliers = nInliers (the count when
 * converged, else 0), T12 = mBestT12 row-major (what iterate returns when it converged, and the best so far when it did not),
 * R / t / s / n_best_inliers = GetEstimatedRotation / Translation / Scale and mnBestInliers, best_iteration = the iteration (from
 * 1) that set them.  inliers[p][n] = vbInliers: all 0 unless converged, then mvbInliersi scattered through mvnIndices1;
 * best_inliers[p][n] (best_inliers may be NULL) = mvbBestInliers scattered the same way; entries with valid == 0 are written 0.
 * hypothesis_inliers[p][max_iterations] (may be NULL): mnInliersi of every evaluated iteration, effective_iterations entries -
 * those behind the stop included; the rest is untouched.
 * A problem with N < min_inliers has no job (:225-229): no_more = 1, identity, s = 1, no inliers, 0 iterations,
 * effective_iterations = 0; a call without a job makes no launch.
 * FT_ERR_INVALID: null arrays, n outside [0, 2^16), an unknown camera model, Tcw1.q / Tcw2.q not a unit quaternion, probability
 * outside (0, 1), min_inliers < 0, max_iterations < 1, a draw outside [0, FT_SIM3_RAND_MAX], n_problems outside [0, 2^16), and
 * min_inliers <= N < 3 (the reference draws from an empty list).  FT_ERR_CAPACITY: max_iterations > FT_SIM3_MAX_ITERATIONS (the
 * reference's call site asks for 300).  Nothing is written on an error.
 * ---------------------------------------------------------------------------------------------- */
#define FT_SIM3_MAX_ITERATIONS 1024
#define FT_SIM3_RAND_MAX 2147483647 /* RAND_MAX of the reference's platform (glibc) */
typedef struct ft_sim3_problem {
    int n;                    /* mN1 = vpMatched12.size() */
    const uint8_t *valid;     /* [n] the pair survived :73-91 */
    const float *world_pos1;  /* n x 3 pMP1->GetWorldPos(); read where valid */
    const float *world_pos2;  /* n x 3 pMP2->GetWorldPos() */
    const float *sigma2_1;    /* [n] pKF1->mvLevelSigma2[kp1.octave] */
    const float *sigma2_2;    /* [n] pKFm->mvLevelSigma2[kp2.octave] */
    ft_se3 Tcw1, Tcw2;        /* pKF1->GetPose(), pKF2->GetPose() */
    int cam_model1;           /* 0 Pinhole, 1 KannalaBrandt8: pKF1->mpCamera */
    float cam1[8];
    int cam_model2;           /* pKF2->mpCamera */
    float cam2[8];
    int fix_scale;            /* bFixScale */
    double probability;       /* SetRansacParameters: 0.99 */
    int min_inliers;          /* nBoWInliers */
    int max_iterations;       /* 300 */
    const int *rand_draws;    /* [3 * max_iterations] rand() */
} ft_sim3_problem;
typedef struct ft_sim3_result {
    int converged, no_more, iterations, effective_iterations;
    int n_inliers, n_best_inliers, best_iteration;
    float T12[16];
    float R[9], t[3], s;
} ft_sim3_result;
FT_API int ft_sim3_solver(ft_context *ctx, int n_problems, const ft_sim3_problem *problems /* [n_problems] */,
                          ft_sim3_result *results /* [n_problems] */, uint8_t *const *inliers /* [n_problems] of [n] */,
                          uint8_t *const *best_inliers /* [n_problems] of [n], or NULL */,
                          int *const *hypothesis_inliers /* [n_problems] of [max_iterations], or NULL */);

/* ------------------------------------------------------------------------------------------------
 * ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint *> &vpMapPoints, th, bRight) (src/ORBmatcher.cc:1247-1437) and
 * ORBmatcher::Fuse(KeyFrame *pKF, Sophus::Sim3f &Scw, vpPoints, th, vpReplacePoint) (:1439-1554): the searches
 * LocalMapping::SearchInNeighbors runs for each of its 20 - 40 target keyframes and both cameras, then for the current keyframe
 * (src/LocalMapping.cc:772-803), and LoopClosing::SearchAndFuse for every keyframe of the corrected window (src/LoopClosing.cc:2133,
 * :2178) - here ONE list of map points against every target (keyframe, camera) of a call.
 * For point i the reference leaves at the first test that fails; stage[i] reports which (0 = the candidate loop was reached):
 *   1  !pMP, isBad(), IsInKeyFrame(pKF) / spAlreadyFound.count(pMP) (:1280-1295, :1464): valid[i] == 0
 *   2  p3Dc = Tcw * p3Dw in the Sophus form (as ft_search_last_frame_se3), p3Dc.z < 0.0f (:1301; z == +-0 passes, invz = 1 / z)
 *   3  uv = pCamera->project(p3Dc) (cam, or cam2 when right) fails KeyFrame::IsInImage: x >= mnMinX && x < mnMaxX && y >= mnMinY
 *      && y < mnMaxY (src/KeyFrame.cc:750-753; a NaN fails)
 *   4  dist3D = (p3Dw - Ow).norm() outside [0.8f * min_distance, 1.2f * max_distance] (:1326)
 *   5  PO.dot(Pn) < 0.5 * dist3D, compared in double (:1334)
 *   6  KeyFrame::GetFeaturesInArea(u, v, th * mvScaleFactors[PredictScale(dist3D, pKF)], bRight) is empty (src/KeyFrame.cc:704-748:
 *      the cells, cell order and box of Frame::GetFeaturesInArea WITHOUT a level filter)
 * The candidate loop (:1359-1408) keeps the keypoints of octave [level - 1, level]; with check_reprojection those that pass
 * (double)(e2 * inv_level_sigma2[octave]) > 7.8 where mvuRight[idx] >= 0 (e2 = ex ex + ey ey + er er, ur = u - mbf * invz) or
 * > 5.99 otherwise (e2 = ex ex + ey ey), every float operation rounded on its own; and takes the smallest DescriptorDistance,
 * strictly: of equal distances the first in GetFeaturesInArea's order (cell column, cell row, index).  With right the keypoints
 * are keys_right, the descriptor rows and best_idx are idx + NLeft.
 * best_idx / best_dist [k * M + i] = bestIdx / bestDist as the loop leaves them for target k: -1 / 256 where no candidate passed or
 * the point left before the loop (the INT_MAX of the Sim3 overload reads 256 too); n_found[k] = points with best_dist <= TH_LOW (50).
 * The map bookkeeping behind the loop (Replace, AddObservation, AddMapPoint, vpReplacePoint, :1411-1430) stays with the caller: it
 * changes nothing a later point's search reads, only which later points test 1 skips - so the caller applies the results in index
 * order and re-tests 1 at that moment, which is exact for one target.  ACROSS targets MapPoint::Replace recomputes the surviving
 * point's descriptor (src/MapPoint.cc:297): the call computes, per target, exactly what Fuse computes FOR THE ARRAYS AS GIVEN; a
 * caller that wants the reference's sequence applies target by target and re-issues a one-target call with valid restricted to the
 * points whose descriptor or position changed.
 * Of the keyframe view N, Nleft, the bounds and grid constants, mbf, keys / keys_right, descriptors, uright (Nleft == -1 only),
 * cam_model, cam, scale_factors and nlevels are read; nothing is written.
 * Launches per call: 2 whatever n_targets, M and the keyframes hold (every target's grid; every (target, point)), one copy up, one
 * copy down, one wait; kernel timing names them kernel.fuse_grid / kernel.fuse_search; statistics fuse.total, fuse.launches.
 * n_targets == 0 or M == 0 returns without a launch (n_found = 0); a target with N == 0 gives -1 / 256 and the stages its points
 * reach.  FT_ERR_INVALID: null arrays, right on a view with Nleft == -1, an unknown camera model, a keypoint octave outside
 * [0, nlevels), check_reprojection without inv_level_sigma2, th <= 0, Tcw.q not a unit quaternion.  Limits (FT_ERR_INVALID beyond
 * them): M < 2^22, n_targets < 2^16, N < 2^24 per keyframe; no other capacity: a window may hold any number of keypoints.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_fuse_points { /* shared by all targets of a call */
    int M;
    const float *world_pos;     /* M x 3 GetWorldPos() */
    const float *normal;        /* M x 3 GetNormal() */
    const float *max_distance;  /* mfMaxDistance (1.2f applied inside, as in ft_map_points) */
    const float *min_distance;  /* mfMinDistance (0.8f inside) */
    const uint8_t *descriptors; /* M x 32 GetDescriptor() */
} ft_fuse_points;
typedef struct ft_fuse_target {
    const ft_frame_view *kf;       /* the keyframe as a frame view (see above) */
    int right;                     /* bRight: project with cam2, search mGridRight / mvKeysRight, bestIdx += NLeft */
    float cam2[8];                 /* mpCamera2, read when right != 0 */
    ft_se3 Tcw;                    /* GetPose() / GetRightPose(); Sim3 form: SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()) */
    float Ow[3];                   /* GetCameraCenter() / GetRightCameraCenter(); Sim3 form: Tcw.inverse().translation() */
    float log_scale_factor;        /* pKF->mfLogScaleFactor */
    const float *inv_level_sigma2; /* [nlevels] mvInvLevelSigma2, read when check_reprojection != 0 */
    const uint8_t *valid;          /* [M] test 1 as it stands at call time; NULL = all */
    float th;                      /* 3.0 in Local Mapping, 4 in Loop Closing */
    int check_reprojection;        /* 1: Fuse(pKF, vpMapPoints, th, bRight); 0: Fuse(pKF, Scw, ...) (no chi-square test) */
} ft_fuse_target;
FT_API int ft_fuse_search(ft_context *ctx, const ft_fuse_points *P, int n_targets, const ft_fuse_target *targets /* [n_targets] */,
                          int *best_idx /* n_targets x M */, int *best_dist /* n_targets x M */, uint8_t *stage /* n_targets x M, may be NULL */,
                          int *n_found /* [n_targets] */);

/* ------------------------------------------------------------------------------------------------
 * ORBmatcher::SearchByProjection(KeyFrame *pKF, Sophus::Sim3f &Scw, vpPoints, vpMatched, th, ratioHamming) (src/ORBmatcher.cc:526-631)
 * and its overload with vpPointsKFs / vpMatchedKF (:633-745), the matchers behind LoopClosing::FindMatchesByProjection
 * (src/LoopClosing.cc:755, :777, :964): the map points of a covisibility window projected into ONE keyframe - here n_jobs
 * independent searches against that keyframe in one call (the loop and the merge detection of NewDetectCommonRegions on the current
 * keyframe; the candidates of DetectCommonRegionsFromBoW).  A job is one call of the reference.
 * For point i in index order the reference leaves at the first test that fails; stage[i] reports which, with the codes 1 - 6 of
 * ft_fuse_search (1 valid[i] == 0: isBad() || spAlreadyFound.count(pMP), the set built from vpMatched ON ENTRY; 2 depth; 3
 * KeyFrame::IsInImage; 4 distance range; 5 viewing angle; 6 KeyFrame::GetFeaturesInArea(u, v, th * mvScaleFactors[level]) of the
 * left camera is empty), 7 = the window held keypoints and the point wrote nothing, 0 = the point wrote.  Tests 2 - 5 and the level
 * are those of the Sim3 overload of Fuse.  hand_pinhole selects the projection: 0 = pKF->mpCamera->project(p3Dc) (:564; cam_model /
 * cam of the view), 1 = invz = 1 / z, x = X * invz, u = fx * x + cx written out (:672-677; cam[0..3] whatever cam_model is, every
 * operation rounded on its own) - the only difference between the overloads a search can see; vpMatchedKF[idx] = vpPointsKFs[iMP]
 * follows from point_keypoint.
 * Among the window's keypoints with matched[idx] == -1 - on entry, and not written by an earlier point of this job - and octave
 * in [level - 1, level] the point takes the smallest DescriptorDistance, strictly: of equal distances the first in
 * GetFeaturesInArea's order (cell column, cell row, index); it writes when (float)bestDist <= (float)TH_LOW * ratio_hamming.  The
 * host turns that into the integer threshold: the largest d of 0 .. 255 with (float)d <= 50.0f * ratio_hamming.
 * matched [N] in / out: -1 = NULL on entry, anything else = held; on return the entries this job wrote hold the point's index, every
 * other entry - all of [Nleft, N) of a two-camera keyframe among them - is unchanged.  point_keypoint[i] (may be NULL) = the
 * keypoint point i wrote, or -1; n_matches = the return value.  bestDist / bestIdx "as the loop leaves them" are not reported.
 * Of the keyframe view N, Nleft, the bounds and grid constants, keys, descriptors, cam_model, cam, scale_factors and nlevels are
 * read; nothing of it is written.
 * Launches per call: 3 whatever n_jobs and the jobs hold (the keyframe's grid; every (job, point): the tests, the window, the
 * candidates within the threshold; a workgroup per job walks the points that have candidates in index order), one copy up, one
 * copy down, one wait; kernel timing names them kernel.sim3_grid / kernel.sim3_candidates / kernel.sim3_resolve; statistics
 * sim3.total, sim3.launches.  n_jobs == 0, every M == 0, or no left keypoints: no launch, n_matches = 0, matched untouched,
 * point_keypoint = -1 and stage = 6 (the tests in front of the window are not made).
 * FT_ERR_INVALID: null arrays, th <= 0, 50 * ratio_hamming < 0 or >= 256 or NaN (the reference would write vpMatched[-1]), Tcw.q
 * not a unit quaternion, a keypoint octave outside [0, nlevels), an unknown camera model, M >= 2^22, n_jobs >= 2^16, N >= 2^24.
 * FT_ERR_CAPACITY, with no output written: more than 1 228 800 left keypoints (a taken bit per keypoint in 150 KB of LDS).  No
 * other capacity: a window may hold any number of candidates.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ft_sim3_job {
    ft_fuse_points points;    /* vpPoints as arrays */
    const uint8_t *valid;     /* [M] !isBad() && !spAlreadyFound.count(pMP); NULL = all */
    ft_se3 Tcw;               /* SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()) */
    float Ow[3];              /* Tcw.inverse().translation() */
    float log_scale_factor;   /* pKF->mfLogScaleFactor */
    int th;                   /* 8, 5, 3 in Loop Closing */
    float ratio_hamming;      /* 1.5, 1.0 */
    int hand_pinhole;         /* 0: the overload of :526 (mpCamera->project); 1: the overload of :633 (written out) */
    int *matched;             /* [N] in / out, see above */
    int *point_keypoint;      /* [M] out, may be NULL */
    uint8_t *stage;           /* [M] out, may be NULL */
    int n_matches;            /* out */
} ft_sim3_job;
FT_API int ft_search_keyframe_sim3(ft_context *ctx, const ft_frame_view *kf, int n_jobs, ft_sim3_job *jobs /* [n_jobs] */);

/* ----------------------------------------------------------------------------------------------
 * MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:329-403) for n_points map points in one call: the producer of the
 * representative descriptor (pMP->GetDescriptor()) every matcher above reads.  The reference calls it in loops over independent
 * points - every map point of a new keyframe (LocalMapping::ProcessNewKeyFrame, src/LocalMapping.cc:312-323), the same points
 * again behind the two Fuse calls of SearchInNeighbors (:806-816), every triangulated point (:704), and the loop-closing and
 * map-creation sites (src/LoopClosing.cc:1130, src/Tracking.cc:2447, 2468, 2616, 3442) - so one call for all of them computes
 * what the loop does.
 * Point p owns descriptors[obs_offsets[p] .. obs_offsets[p + 1]): vDescriptors in the caller's order, i.e. the rows the loop at
 * :348-363 pushes - over the observation map, keyframes with isBad() skipped (:352), the left index first (:356-358), then the
 * right index (:359-361).  The caller gathers them: the map bookkeeping stays with the caller, as for ft_fuse_search.
 * With N the length of the list, d(i, j) = ORBmatcher::DescriptorDistance (:377) and row i = d(i, 0 .. N - 1), the 0 of the
 * diagonal included (:374):
 *   median(i)  = the element at index (size_t)(0.5 * (N - 1)) = (N - 1) / 2 of the ascending-sorted row (:388-390): the LOWER
 *                median of an even N;
 *   BestIdx    = the first i with the smallest median: it starts at 0 (:385) and the compare is a strict < (:392);
 *   best_index[p] = BestIdx, best_median[p] = BestMedian (:394-395), out_descriptors[p] = vDescriptors[BestIdx] (:401).
 * N == 0: the reference returns at :365 (or at :343) without touching mDescriptor; here best_index[p] = -1, best_median[p] = -1
 * and the 32 bytes of out_descriptors[p] stay as the caller passed them.
 * A distance reaches 256 (a descriptor and its complement); no step holds a distance in a byte.
 * Per-point cap: a list holds at most FT_DISTINCT_MAX_OBSERVATIONS (1 024) descriptors.  (The reference keeps float
 * Distances[N][N] on the stack, :371, and dies near N = 1 400 under the default 8 MB stack.)
 * Launches per call: at most 3, whatever n_points - one per length class that occurs (N <= 16: several points per wave; N <= 64:
 * a wave per point; longer: a workgroup per point), one copy up, one copy down, one wait; kernel timing names them
 * kernel.distinct_short / kernel.distinct_wave / kernel.distinct_block; statistics distinctive_descriptors.total,
 * distinctive_descriptors.launches.  n_points == 0 or every list empty: no launch (best_index / best_median are still filled
 * with -1).  There is no CPU path.
 * FT_ERR_INVALID: null ctx, obs_offsets or best_index; descriptors null while obs_offsets[n_points] > 0; n_points < 0;
 * obs_offsets[0] != 0 or a decreasing offset.  FT_ERR_CAPACITY, ft_last_error() naming the point: a list longer than the cap; a
 * call whose arena (the descriptors, 48 bytes per point) would pass 4 GB.  No output is written on an error, and descriptors is
 * not read before every offset has been checked.
 * ---------------------------------------------------------------------------------------------- */
#define FT_DISTINCT_MAX_OBSERVATIONS 1024
FT_API int ft_distinctive_descriptors(ft_context *ctx, int n_points,
                                      const int *obs_offsets /* [n_points + 1], obs_offsets[0] == 0, non-decreasing */,
                                      const uint8_t *descriptors /* obs_offsets[n_points] x 32 bytes, host */,
                                      int *best_index /* [n_points] */, int *best_median /* [n_points] or NULL */,
                                      uint8_t *out_descriptors /* n_points x 32 bytes or NULL */);

/* ----------------------------------------------------------------------------------------------
 * KeyFrameDatabase (src/KeyFrameDatabase.cc), device-resident: the step of the BoW chain between ft_bow_transform (a keyframe's
 * BowVector) and ft_search_by_bow_keyframes / ft_search_by_bow (which consume the candidates of a place-recognition query).
 * Ported are the two queries with a caller: DetectNBestCandidates (:604-730; LoopClosing.cc:491) and
 * DetectRelocalizationCandidates (:733-845; Tracking.cc:3810), with L1Scoring::score
 * (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  DetectCandidates, DetectBestCandidates and DetectLoopCandidates have no
 * caller and stay out.
 *
 * There is no inverted file: a wave per stored keyframe intersects two sorted word lists, so add is an append and erase a
 * tombstone.  A HANDLE is the add sequence number of a keyframe (0, 1, 2, ... over the database's lifetime; never reused).
 * ft_kfdb_create: scoring uses the reference's enum (BowVector.h); 0 (L1_NORM, what ORBvoc uses) is implemented, anything else
 *   is FT_ERR_INVALID.  The database counts as an object of its context: ft_context_destroy refuses while it is alive.
 * ft_kfdb_add (:39-45): n BowVectors in CSR form - keyframe k owns bow_ids / bow_values [bow_offsets[k], bow_offsets[k + 1]),
 *   ids strictly ascending, exactly what ft_bow_transform returns; a vector may be empty.  handles_out[k] = its handle.  Ids and
 *   values are stored in two device arrays; storage grows by doubling and keeps its contents.
 * ft_kfdb_erase (:47-66): a tombstone.  An unknown or already erased handle (also: twice in one call) is FT_ERR_INVALID and
 *   nothing is erased.  clearMap (:74-98) is an erase of that map's handles.  KeyFrame::SetBadFlag erases (KeyFrame.cc:678), so
 *   the database never holds a bad keyframe: the isBad() test at :712 is the caller's.  When the words of erased keyframes
 *   exceed half of the stored words, the rows are compacted in handle order (statistic kfdb.compactions).
 * ft_kfdb_clear (:68-72): every keyframe goes; handles keep counting.
 * ft_kfdb_size: live keyframes and the words they hold.
 *
 * Per keyframe and per query KIND (0 place recognition: mnPlaceRecognitionQuery / mnPlaceRecognitionWords /
 * mPlaceRecognitionScore; 1 relocalisation: mnRelocQuery / mnRelocWords / mRelocScore) the database keeps the reference's three
 * members, 0 when a keyframe is added (KeyFrame.cc:33-34).  THEY PERSIST BETWEEN QUERIES, as in the reference: :689 adds the
 * stored score of a neighbour that was stamped by this query but not scored in it - whatever an earlier query left.
 * ft_kfdb_state reads them (from the host mirror the last query of that kind left; no device access).
 *
 * ft_kfdb_score: the device part of a query, :615-666 (kind 0, with the connected set spConnectedKF as handles) or :741-787
 *   (kind 1, n_connected must be 0).  For every live keyframe that shares at least one word with the query: a stamp that differs
 *   from query_id resets the count, and the keyframe - unless connected - is stamped and LISTED; the count then grows by the
 *   shared words.  A connected keyframe ends with count 1 and its stamp unchanged; a keyframe already stamped with query_id is
 *   not listed again and its count accumulates.  maxCommonWords is taken over the listed keyframes,
 *   minCommonWords = (int)(maxCommonWords * 0.8f) (one fp32 product, truncated), and a listed keyframe is scored when its
 *   count is strictly greater.  The score: the terms (|vi - wi| - |vi|) - |wi| of the common words, vi the query's value, added
 *   in ascending word order into one double; -sum / 2.0; rounded to float; written to the keyframe's state.
 *   Outputs: n_sharing (listed keyframes), max_common_words, min_common_words, n_scored, and for the scored keyframes, in the
 *   order of lKFsSharingWords (first encounter walking the query's words ascending and each word's list in insertion order =
 *   ascending (first shared word, handle)): scored_handles, scored_words, scored_scores and - may be NULL - raw_scores, the
 *   double before the rounding to float.  Each array holds up to n_live entries.
 *   One block up, TWO launches whatever the number of keyframes or words (kernel.kfdb_count, kernel.kfdb_score), the records and
 *   the state of the kind down, one wait; statistics kfdb_score.total, kfdb_score.launches.  n_words == 0, an empty database or
 *   one whose keyframes hold no word: zeros without a launch.
 *   FT_ERR_INVALID: query ids not strictly ascending, a connected handle that is not live, null arrays with non-zero counts,
 *   kind outside {0, 1}.  FT_ERR_CAPACITY: a query of more than FT_KFDB_MAX_QUERY_WORDS words (2 x nFeatures = 4 000 fits).
 *
 * The selection calls are host code (no launch, no device access); they read the state the scoring call left.  They need
 * GetBestCovisibilityKeyFrames(10) and GetMap() of the SCORED keyframes only, which the caller gathers: neighbours of scored
 * keyframe i are neigh_handles[neigh_offsets[i] .. neigh_offsets[i + 1]) in the reference's order, maps are any integer labels.
 * ft_kfdb_select_n_best (:671-729): float accumulation over the neighbours in the given order; a neighbour counts only when its
 *   stamp equals query_id and then adds its STORED score; pBestKF moves on a strict >; a STABLE descending sort on the
 *   accumulated score; the walk deduplicates by keyframe, splits loop (same map as query_map) from merge candidates, skips
 *   merge candidates of a map in bad_maps and stops when both lists hold n_candidates.  loop_out / merge_out hold n_candidates.
 * ft_kfdb_select_reloc (:792-844): the same accumulation on the relocalisation state; minScoreToRetain = 0.75f * bestAccScore;
 *   entries strictly greater, in list order (no sort), of the given map, deduplicated.  out holds n_scored.
 * A scored or neighbour handle that is erased or unknown is FT_ERR_INVALID.
 * ---------------------------------------------------------------------------------------------- */
#define FT_KFDB_MAX_QUERY_WORDS 4096
#define FT_KFDB_PLACE_RECOGNITION 0
#define FT_KFDB_RELOCALIZATION 1
typedef struct ft_kfdb ft_kfdb;
FT_API int ft_kfdb_create(ft_context *ctx, int scoring, ft_kfdb **out);
FT_API int ft_kfdb_destroy(ft_kfdb *db);
FT_API int ft_kfdb_add(ft_kfdb *db, int n, const int *bow_offsets /* [n + 1], bow_offsets[0] == 0 */, const unsigned *bow_ids,
                       const double *bow_values, int *handles_out /* [n] */);
FT_API int ft_kfdb_erase(ft_kfdb *db, int n, const int *handles);
FT_API int ft_kfdb_clear(ft_kfdb *db);
FT_API int ft_kfdb_size(const ft_kfdb *db, int *n_live, long long *n_words);
FT_API int ft_kfdb_state(const ft_kfdb *db, int kind, int n, const int *handles, long long *stamps /* [n] or NULL */,
                         int *words /* [n] or NULL */, float *scores /* [n] or NULL */);
FT_API int ft_kfdb_score(ft_kfdb *db, int kind, long long query_id, int n_words, const unsigned *ids, const double *values,
                         int n_connected, const int *connected_handles, int *n_sharing, int *max_common_words,
                         int *min_common_words, int *n_scored, int *scored_handles /* [n_live] */, int *scored_words /* [n_live] */,
                         float *scored_scores /* [n_live] */, double *raw_scores /* [n_live] or NULL */);
FT_API int ft_kfdb_select_n_best(const ft_kfdb *db, long long query_id, int n_scored, const int *scored_handles,
                                 const float *scored_scores, const int *neigh_offsets /* [n_scored + 1] */, const int *neigh_handles,
                                 const int *scored_map /* [n_scored] */, const int *neigh_map, int query_map, int n_bad_maps,
                                 const int *bad_maps, int n_candidates, int *loop_out, int *n_loop, int *merge_out, int *n_merge);
FT_API int ft_kfdb_select_reloc(const ft_kfdb *db, long long query_id, int n_scored, const int *scored_handles,
                                const float *scored_scores, const int *neigh_offsets /* [n_scored + 1] */, const int *neigh_handles,
                                const int *scored_map /* [n_scored] */, const int *neigh_map, int map, int *out /* [n_scored] */,
                                int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* FASTTRACK_AMD_H */
