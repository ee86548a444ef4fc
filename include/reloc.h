/* reloc.h -- C-ABI of libreloc_hip.so, the MI355X (gfx950) visual-relocalization library.
 *
 * The reference (vbronetskyi/nclt-slam-project) has no FFI for this path: its boundary is the
 * Python `cv2` API at the call sites listed below, with OpenCV's CPU code underneath.  This
 * header DEFINES the C-ABI that replaces that native layer; every entry point cites the
 * reference call it serves (paths relative to simulation/isaac/ in the reference tree):
 *   M = scripts/common/visual_landmark_matcher.py     R = scripts/common/visual_landmark_recorder.py
 *   G = experiments/63_global_reloc/scripts/visual_landmark_matcher.py
 *   S = experiments/55_visual_teach_repeat/scripts/checkpoint_a_selftest.py
 * The Python binding a maintainer adds is shown in INTEGRATION.md; the shipped one is
 * nclt-slam-project_amd/_native.py.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no framework types.
 *   - every function returns 0 on success or a negative RELOC_E_* code; reloc_last_error()
 *     gives the message of the calling thread's last failure.
 *   - a reloc_ctx owns one HIP stream, its scratch buffers and (optionally) one uploaded
 *     landmark database.  A ctx is not thread-safe; any number of ctxs may coexist.
 *   - functions without a suffix take HOST pointers, run synchronously and return results in
 *     caller-allocated host memory (what the cv2-shaped Python layer needs).
 *   - functions ending in _dev take DEVICE pointers (hipMalloc / reloc_dev_alloc / a torch
 *     tensor's data_ptr()), enqueue on the ctx stream and return without synchronising.
 *   - there is NO CPU fallback: every compute entry point fails with RELOC_E_NODEVICE when no
 *     gfx950 device is usable.
 */
#ifndef RELOC_H
#define RELOC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RELOC_OK            0
#define RELOC_E_ARG        (-1)   /* bad argument (cv2.error in the Python layer)          */
#define RELOC_E_NODEVICE   (-2)   /* no usable HIP device                                  */
#define RELOC_E_HIP        (-3)   /* HIP runtime error, see reloc_last_error()             */
#define RELOC_E_CAPACITY   (-4)   /* input exceeds a ctx capacity                          */
#define RELOC_E_STATE      (-5)   /* call needs state that is missing (e.g. no database)   */

#define RELOC_ORDER_BGR 0
#define RELOC_ORDER_RGB 1

/* outcome codes of reloc_tick, one per CSV outcome string of M:308,313,383,395,428 */
#define RELOC_OUT_PUBLISHED        0
#define RELOC_OUT_NO_FEATURES      1   /* curr_no_features  */
#define RELOC_OUT_NO_CANDIDATES    2   /* no_candidates     */
#define RELOC_OUT_NO_PNP_ACCEPT    3   /* no_pnp_accept     */
#define RELOC_OUT_CONSISTENCY_FAIL 4   /* consistency_fail_ */

typedef struct reloc_ctx reloc_ctx;

/* Matcher parameters of the fused tick: the module-level constants of the reference matcher (M:56-75, accumulation
 * M:85-89, global relocalisation G:80-86).  reloc_create() installs the reference's values; a host that runs with
 * other values (MatcherConfig in the Python layer) sets them here, so the fused device tick and the cv2-shaped path
 * gate identically. */
typedef struct reloc_params {
    int32_t nfeatures;               /* ORB_create(nfeatures)                 M:207   500   */
    int32_t max_candidates;          /* MAX_CANDIDATES (<= 10)                M:57    5     */
    int32_t min_matches;             /* MIN_MATCHES                           M:65    10    */
    int32_t min_inliers;             /* MIN_INLIERS                           M:70    10    */
    int32_t ransac_iterations;       /* RANSAC_ITERATIONS (<= 1024)           M:69    200   */
    int32_t global_max_candidates;   /* RELOC_MAX_CANDIDATES (<= 32)          G:84    25    */
    int32_t global_min_inliers;      /* RELOC_MIN_INLIERS                     G:85    18    */
    int32_t accum_min_kpts;          /* ACCUM_MIN_KPTS                        M:88    30    */
    double candidate_radius_m;       /* CANDIDATE_RADIUS_M                    M:56    8.0   */
    double heading_tol_deg;          /* HEADING_TOL_DEG                       M:58    90.0  */
    double reproj_max_px;            /* REPROJ_ERR_MAX_PX                     M:67    2.0   */
    double ransac_reproj_px;         /* RANSAC_REPROJ_PX                      M:68    3.0   */
    double ransac_confidence;        /* cv2.solvePnPRansac default                    0.99  */
    double consistency_m;            /* CONSISTENCY_M                         M:75    5.0   */
    double global_reproj_max_px;     /* RELOC_REPROJ_MAX_PX                   G:86    1.5   */
    double accum_min_dist_m;         /* ACCUM_MIN_DIST_M                      M:87    5.0   */
    double accum_depth_min_m;        /* d_c > 0.5                             M:461   0.5   */
    double accum_depth_max_m;        /* d_c < 15.0                            M:461   15.0  */
    int32_t gray_coeff_bits;         /* BGR2GRAY fixed point: 15 or 14 (reloc_spec.h) M:305  15    */
    int32_t reserved0;               /* must be 0                                                  */
} reloc_params;

/* ---- lifetime, errors, plumbing ----------------------------------------------------------- */
const char *reloc_last_error(void);
int  reloc_device_count(void);
/* max_w/max_h: largest frame; max_feat: largest keypoint / descriptor count per frame. */
reloc_ctx *reloc_create(int device, int max_w, int max_h, int max_feat);
void reloc_destroy(reloc_ctx *ctx);
/* Use an externally owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL
 * restores the ctx's own stream. */
int  reloc_set_stream(reloc_ctx *ctx, void *hip_stream);
int  reloc_sync(reloc_ctx *ctx);
void *reloc_dev_alloc(reloc_ctx *ctx, int64_t bytes);
int  reloc_dev_free(reloc_ctx *ctx, void *p);
int  reloc_h2d(reloc_ctx *ctx, void *dst_dev, const void *src_host, int64_t bytes);   /* async */
int  reloc_d2d(reloc_ctx *ctx, void *dst_dev, const void *src_dev, int64_t bytes);    /* async */
/* Pinned (page-locked) host memory for frames and results: copies from / to it are true DMA and overlap with kernels. */
void *reloc_host_alloc(int64_t bytes);
int  reloc_host_free(void *p);
/* The ctx's current hipStream_t (to order work of other libraries against it). */
void *reloc_get_stream(reloc_ctx *ctx);
int  reloc_d2h(reloc_ctx *ctx, void *dst_host, const void *src_dev, int64_t bytes);   /* async */
/* HIP-event stopwatch on the ctx stream: begin(); ...launches...; end() -> ms (synchronises). */
int  reloc_timer_begin(reloc_ctx *ctx);
int  reloc_timer_end(reloc_ctx *ctx, float *ms);
/* Per-kernel stopwatch: when enabled, the dominant kernels are bracketed by HIP events on the
 * ctx stream; get() synchronises and returns total ms and launch count of kernel `which`. */
#define RELOC_PROF_DB_SCAN  0
#define RELOC_PROF_MATRIX   1
#define RELOC_PROF_ORB      2
#define RELOC_PROF_PNP      3
#define RELOC_PROF_STEREO   4   /* k_stereo_depth (reloc_stereo_depth and the stereo recording / accumulation) */
#define RELOC_PROF_STEREO_DENSE 5 /* k_stereo_dense + k_stereo_dense_finish with the right map's reset (the dense stereo entry points) */
#define RELOC_PROF_N        6   /* the slots above */
#define RELOC_PROF_STEREO_SGM 6 /* the semi-global dense pass: both resets, volume, paths, selection, finish (and the speckle stage) */
#define RELOC_PROF_COUNT    7   /* every slot: reloc_profile_get takes 0 <= which < RELOC_PROF_COUNT */
int  reloc_profile_enable(reloc_ctx *ctx, int on);
int  reloc_profile_get(reloc_ctx *ctx, int which, float *total_ms, int32_t *launches);

int  reloc_get_params(reloc_ctx *ctx, reloc_params *out);
int  reloc_set_params(reloc_ctx *ctx, const reloc_params *p);

/* ---- ORB front end ------------------------------------------------------------------------ */
/* cv2.cvtColor(img, COLOR_BGR2GRAY)                                         M:305  R:240  S:44 */
int reloc_gray_u8(reloc_ctx *ctx, const uint8_t *img, int w, int h, int stride, int order,
                  uint8_t *gray);
/* cv2.ORB_create(nfeatures).detectAndCompute(gray, None)                    M:306  R:241  S:48
 * Outputs hold up to the ctx's max_feat rows; *n_out = rows written.  Keypoints are level-major,
 * raster order inside a level.  xy = KeyPoint.pt (level-0 pixels), octave = pyramid level. */
int reloc_orb_detect_compute(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride,
                             int nfeatures, float *xy, float *size, float *angle, float *response,
                             int32_t *octave, uint8_t *desc, int32_t *n_out);
/* Same from a 3-channel frame already in device memory (gray conversion fused in front);
 * results stay in ctx-owned device buffers (see reloc_frame_*).  Enqueue only. */
int reloc_orb_frame_dev(reloc_ctx *ctx, const uint8_t *img_dev, int w, int h, int stride, int order,
                        int nfeatures);
/* Device views of the last frame's features (valid until the next frame call). */
const uint8_t *reloc_frame_desc_dev(reloc_ctx *ctx);      /* max_feat x 32 u8                  */
const float   *reloc_frame_xy_dev(reloc_ctx *ctx);        /* max_feat x 2 f32                  */
const int32_t *reloc_frame_count_dev(reloc_ctx *ctx);     /* 1 x i32: number of keypoints      */
/* Debug/parity taps: copy intermediate planes of the last frame to host.  level in [0, 8).
 * what: 0 = pyramid level, 1 = blurred level, 2 = NMS-kept FAST score map. */
int reloc_frame_debug_plane(reloc_ctx *ctx, int what, int level, uint8_t *out, int32_t *w, int32_t *h);
/* The stage record of the last frame, 8 x i32 each: the stage-1 cut score of every level (-1 where the level's NMS map is
 * empty, so that no cut was computed), the length of its stage-1 candidate list and the number of keypoints kept of it.
 * Read only; synchronises the stream. */
int reloc_orb_debug_levels(reloc_ctx *ctx, int32_t *cut, int32_t *cand_cnt, int32_t *kp_cnt);

/* ---- ORB detection mask (include/reloc_spec.h, "ORB MASK") ---------------------------------------- */
/* cv2.ORB.detectAndCompute(image, mask): mask is a host plane of h rows of w bytes, stride bytes apart; a corner is kept
 * where its mask level is non-zero, before the per-level quota is spent.  reloc_set_orb_mask keeps a persistent mask on the
 * context; mask == NULL or w == h == 0 turns it off (the default of a new context; the launch sequence is then that of a
 * context that never had one).  The first use allocates the context's two mask pyramids.  The persistent mask has the size
 * of the working frame (behind reloc_set_resize) and is applied by every entry point that goes through the image chain:
 * reloc_orb_frame_dev, reloc_record_frame, reloc_tick, reloc_tick_dev, reloc_tick_batch_dev, reloc_tick_scan_dev,
 * reloc_shard_scan_batch_dev (the accumulation uses the tick's features); a working frame of another size fails with
 * RELOC_E_ARG before anything is launched.  Never applied to the caller's gray plane of reloc_orb_detect_compute.  The
 * contexts of a batched call may hold different masks but agree on masked / unmasked and on the mask size, else
 * RELOC_E_STATE.  reloc_get_orb_mask returns (0, 0) when off. */
int reloc_set_orb_mask(reloc_ctx *ctx, const uint8_t *mask, int w, int h, int stride);
int reloc_get_orb_mask(reloc_ctx *ctx, int32_t *w, int32_t *h);
/* reloc_orb_detect_compute under a mask of the gray plane's size given with the call; the persistent mask and its pyramid
 * stay as they were. */
int reloc_orb_detect_compute_masked(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride, const uint8_t *mask,
                                    int mask_stride, int nfeatures, float *xy, float *size, float *angle,
                                    float *response, int32_t *octave, uint8_t *desc, int32_t *n_out);
/* Parity tap: level (in [0, 8)) of the mask pyramid that the last masked frame used, dense rows of *w bytes. */
int reloc_orb_mask_level(reloc_ctx *ctx, int level, uint8_t *out, int32_t *w, int32_t *h);

/* ---- ORB parameters (include/reloc_spec.h, "ORB PARAMS") ------------------------------------------- */
/* cv2.ORB_create(nfeatures, scaleFactor, nlevels, ..., scoreType, ..., fastThreshold): nlevels 1..8, scale_factor finite in
 * [1.01, 2.0], fast_threshold 1..254, score_type 0 = HARRIS_SCORE | 1 = FAST_SCORE; anything else is RELOC_E_ARG with the
 * range in the message.  A new context holds OpenCV's defaults (8, 1.2, 20, HARRIS_SCORE) and runs the kernels built for
 * them.  reloc_set_orb_params is persistent and used by every entry point that runs ORB: reloc_orb_detect_compute,
 * reloc_orb_detect_compute_masked, reloc_orb_frame_dev, reloc_record_frame, every reloc_tick*, the shard entry points (the
 * accumulation uses the tick's features).  The next frame plans its geometry anew; blocks whose size depends on the scale
 * grow when needed (the stream is drained) and never shrink, and a frame whose plan does not fit what the context holds
 * fails with RELOC_E_CAPACITY before anything is launched.  Levels >= nlevels are empty: reloc_frame_debug_plane and
 * reloc_orb_mask_level return RELOC_OK and 0 x 0 for them.  The contexts of a batched call agree on all four, else
 * RELOC_E_STATE. */
int reloc_set_orb_params(reloc_ctx *ctx, int nlevels, double scale_factor, int fast_threshold, int score_type);
int reloc_get_orb_params(reloc_ctx *ctx, int32_t *nlevels, double *scale_factor, int32_t *fast_threshold, int32_t *score_type);
/* reloc_orb_detect_compute with the four parameters, and under a mask when mask != NULL (as _masked), for this call only:
 * the persistent parameters, the persistent mask and its pyramid stay as they were. */
int reloc_orb_detect_compute_params(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride, const uint8_t *mask,
                                    int mask_stride, int nfeatures, int nlevels, double scale_factor, int fast_threshold,
                                    int score_type, float *xy, float *size, float *angle, float *response,
                                    int32_t *octave, uint8_t *desc, int32_t *n_out);

/* Teach-side record builder (R:240-288): ORB on the frame, then per keypoint the border / ground masks,
 * depth lookup (uint16 millimetres), 3x3 non-zero depth std, range and variance gates and pin-hole
 * back-projection.  Outputs (up to max_feat rows, keypoint order kept): xy = keypoints_2d, desc =
 * descriptors, pts3d = keypoints_3d_cam, kp_index = row in the frame's ORB output.  The caller applies
 * the ">= 30 survivors" rule (R:270) and the displacement trigger. */
int reloc_record_frame(reloc_ctx *ctx, const uint8_t *img, const uint16_t *depth_mm, int w, int h, int order,
                       int nfeatures, float *xy, uint8_t *desc, float *pts3d, int32_t *kp_index,
                       int32_t *n_out, int32_t *n_kp);

/* Depth image -> obstacle points of the relay's depth_cb (scripts/common/tf_wall_clock_relay_v55.py:1020-1038):
 * every `step`-th pixel with zmin < z < zmax, point = (z, -(u-cx)/fx*z, -(v-cy)/fy*z) f32, raster order.
 * depth: float32 metres (is_f32) or uint16 millimetres; points holds ceil(w/step)*ceil(h/step) x 3. */
int reloc_depth_points(reloc_ctx *ctx, const void *depth, int is_f32, int w, int h, int step, const double K4[4],
                       float zmin, float zmax, float *points, int32_t *n_out);

/* ---- 256-bit Hamming matching --------------------------------------------------------------- */
/* cv2.BFMatcher(NORM_HAMMING, crossCheck=True).match(q, t)                  M:211,327  G:337
 * Mutual nearest neighbours, lowest index on ties, sorted by queryIdx.  Outputs sized min(nq,nt). */
int reloc_match_mutual(reloc_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt,
                       int32_t *qidx, int32_t *tidx, int32_t *dist, int32_t *n_out);
/* cv2.BFMatcher(NORM_HAMMING, crossCheck=False).knnMatch(q, t, k=2)         S:46,68
 * idx/dist are nq x 2; a missing second neighbour is (-1, -1). */
int reloc_match_knn2(reloc_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt,
                     int32_t *idx, int32_t *dist);
/* knnMatch(q, t, k=2) + Lowe test in one call: the lists of the MATCH POLICY block of reloc_spec.h (queryIdx = row of q in
 * ascending order, trainIdx = its nearest row of t, distance), outputs sized nq.  ratio: finite, in (0, 1], else RELOC_E_ARG.
 * nq <= 65535 (the capacity of a frame's features), nt < 2^22. */
int reloc_match_ratio(reloc_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, double ratio,
                      int32_t *qidx, int32_t *tidx, int32_t *dist, int32_t *n_out);
/* Match policy of the tick (reloc_spec.h, "MATCH POLICY"): how the candidate records are paired with the frame's features
 * (the match lists and the 3-D / 2-D pairs PnP is given) and what the whole-database search counts per record.  Persists
 * like the other reloc_set_* settings; a new context has (RELOC_MATCH_CROSS, 0.8).  Any other policy, a non-finite ratio or
 * one outside (0, 1]: RELOC_E_ARG.  With RELOC_MATCH_CROSS the ratio is stored and ignored.  Read by every tick entry point
 * (reloc_tick*, reloc_tick_scan_dev / _solve_dev, reloc_shard_scan_batch_dev / _solve_batch_dev); the contexts of a batch must
 * agree (RELOC_E_STATE).  A ratio list holds up to max_feat entries, so under RELOC_MATCH_RATIO a context whose max_feat
 * exceeds 4096 (the stride of the match lists) is refused by the tick entry points with RELOC_E_CAPACITY. */
#define RELOC_MATCH_CROSS 0   /* BFMatcher(crossCheck=True).match(desc_t, desc_curr)          M:211,327 */
#define RELOC_MATCH_RATIO 1   /* knnMatch(desc_curr, desc_t, k=2) + Lowe test                 S:68-71   */
int reloc_set_match_policy(reloc_ctx *ctx, int policy, double ratio);
int reloc_get_match_policy(reloc_ctx *ctx, int32_t *policy, double *ratio);
/* landmarks.pkl -> packed device arena (R:290-297, M:179-187).  desc: T x 32; pts3d: T x 3
 * (keypoints_3d_cam); offsets: L+1 row offsets; poses: L x 7 camera pose (x y z qx qy qz qw).
 * Replaces any previously uploaded database. */
int reloc_db_upload(reloc_ctx *ctx, const uint8_t *desc, const float *pts3d, const int64_t *offsets,
                    const double *poses, int64_t n_records);
int64_t reloc_db_records(reloc_ctx *ctx);
int64_t reloc_db_rows(reloc_ctx *ctx);
/* The database lives in a capacity-reserved arena: appending a record (accumulation, M:435-500) copies its rows behind
 * the last one and never re-allocates while the reserve lasts; reserve() grows the arena (device-to-device copy of
 * the contents) and is also what upload/append call when the reserve is exhausted (geometric growth). */
int reloc_db_reserve(reloc_ctx *ctx, int64_t cap_records, int64_t cap_rows);
/* self.landmarks.append(new_lm); self.xy = vstack(...); self.heading = append(...)        M:489-493
 * desc n x 32, pts3d n x 3 (keypoints_3d_cam), kp2d n x 2 or NULL (keypoints_2d, kept for reloc_db_fetch), pose =
 * camera pose x y z qx qy qz qw, index_xy = the (x, y) the candidate search files the record under (the reference
 * files an accumulated record under the VIO position, M:491; NULL = pose x, y as for taught records M:213). */
int reloc_db_append(reloc_ctx *ctx, const uint8_t *desc, const float *pts3d, const float *kp2d, int n,
                    const double pose[7], const double index_xy[2]);
/* Two resident databases (slot 0 / 1): the split-landmark variant keeps the outbound set in one and the return-leg
 * set in the other and flips at the turnaround (X:274-294).  upload / append / reserve / tick act on the selected
 * slot; selecting costs nothing on the device. */
int reloc_db_select(reloc_ctx *ctx, int slot);
/* Several contexts (streams) on one device scanning ONE resident database: dst adopts the selected database of src
 * (descriptors, points, offsets, poses, index) without copying and keeps only its own per-tick scratch.  The shared
 * database is read-only through dst (append / reserve on dst fail with RELOC_E_STATE).  dst sees the database as it was
 * when it was adopted: records that src appends or accumulates later, and a new upload through src, need a new
 * reloc_db_share to become visible.  The arrays are reference-counted: src may grow past its reserve, upload again or be
 * destroyed at any time -- dst keeps scanning the arrays it adopted, which are freed when their last holder lets go. */
int reloc_db_share(reloc_ctx *dst, reloc_ctx *src);
/* Read one record back (save of the augmented database M:502-514, parity taps).  Any output may be NULL; desc / pts3d /
 * kp2d must hold the record's rows (query *n first with all arrays NULL). */
int reloc_db_fetch(reloc_ctx *ctx, int64_t record, uint8_t *desc, float *pts3d, float *kp2d, double pose[7],
                   double index_xyh[4], int32_t *n);
/* Whole-database scan of G:329-344: per record, the number of mutual matches between the
 * record's descriptors (query) and the current frame's descriptors (train).  cur: n_cur x 32. */
int reloc_db_match_counts(reloc_ctx *ctx, const uint8_t *cur, int n_cur, int32_t *counts);
int reloc_db_match_counts_dev(reloc_ctx *ctx, const uint8_t *cur_dev, const int32_t *n_cur_dev,
                              int n_cur_max, int32_t *counts_dev);
/* Ratio-test score of every record: number of current descriptors whose two nearest rows of the record
 * satisfy d1 < ratio * d2 -- knnMatch(desc_cur, desc_record, k=2) + Lowe test of the archived anchor
 * localizers (_archive/anchor_localizer.py:82-90, ratio 0.75) and the self-test (S:68-71, 0.80). */
int reloc_db_ratio_counts(reloc_ctx *ctx, const uint8_t *cur, int n_cur, double ratio, int32_t *counts);
/* All-pairs u16 distance matrix (loop-closure sweep shape; no reference counterpart,
 * BASELINE.json config 5): out[i * nb + j] = hamming(a_i, b_j). */
int reloc_hamming_matrix(reloc_ctx *ctx, const uint8_t *a, int64_t na, const uint8_t *b, int64_t nb,
                         uint16_t *out);
int reloc_hamming_matrix_dev(reloc_ctx *ctx, const uint8_t *a_dev, int64_t na, const uint8_t *b_dev,
                             int64_t nb, uint16_t *out_dev);

/* ---- PnP ------------------------------------------------------------------------------------ */
/* Hypothesis scorer inside cv2.solvePnPRansac (M:342-346): inlier count of H poses
 * (R row-major 9 + t 3 doubles each) over m correspondences; K4 = fx fy cx cy. */
int reloc_pnp_score(reloc_ctx *ctx, const float *obj, const float *img, int m, const double *Rt, int H,
                    const double K4[4], float thr_px, int32_t *inlier_count, uint8_t *mask);
/* cv2.solvePnPRansac(obj, img, K, DIST, iterationsCount=, reprojectionError=, flags=ITERATIVE)
 *                                                                            M:342-346  S:78-82
 * inliers must hold m entries. */
int reloc_pnp_ransac(reloc_ctx *ctx, const float *obj, const float *img, int m, const double K4[4],
                     int iters, float thr_px, double conf, uint64_t seed, double rvec[3],
                     double tvec[3], int32_t *inliers, int32_t *n_inl, int32_t *ok);
/* Parity tap (tests only): the hypothesis stage of the last PnP launch on ctx, for candidate `slot` -- slot 0 after
 * reloc_pnp_ransac[_dist] (a call with m < 4 launches nothing and leaves the previous launch in place), the slot's order in
 * reloc_tick_debug's cand_ids after a tick solve.  Rt: the first n poses (n x 12 doubles, R row-major | t) as the
 * hypothesis kernel wrote them; cnt: their n inlier counts; *best_h: the hypothesis the RANSAC decision chose (-1: none).
 * A row whose count is -1 holds no pose (the sample was degenerate or no root gave one): its 12 doubles are whatever the
 * buffer held before.  Rows at or beyond the launch's iterationsCount are stale as well.  RELOC_E_ARG for slot outside
 * [0, 32), n outside [1, 1024] or a NULL pointer.  Synchronises the context's stream; copies only, launches nothing. */
int reloc_pnp_debug_hypotheses(reloc_ctx *ctx, int slot, int n, double *Rt, int32_t *cnt, int32_t *best_h);

/* Camera model used by the fused tick: K4 = fx fy cx cy (M:49-52) and the static base_link ->
 * camera transform stored in landmarks.pkl (M:183-184; R:81-88).  NULL keeps the current value;
 * the defaults are the reference's constants. */
int reloc_set_camera(reloc_ctx *ctx, const double K4[4], const double base_to_cam_t[3],
                     const double base_to_cam_R[9]);

/* ---- lens distortion (include/reloc_spec.h, RELOC_UNDISTORT_ITERS) ---------------------------- */
/* OpenCV's default model, coeffs = k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4 [tx ty]]]] with n in {0, 4, 5, 8, 12, 14}; every
 * coefficient after the fifth must be exactly 0 (the rational, thin-prism and tilted models are not implemented) and all
 * must be finite, else RELOC_E_ARG.  n = 0 or all zero: pinhole (the pinhole kernels run, results bit-identical).  A new
 * context is pinhole.  Read by reloc_tick, reloc_tick_dev, reloc_tick_batch_dev, reloc_tick_solve_dev,
 * reloc_shard_solve_batch_dev, reloc_record_frame and reloc_tick_accumulate_dev; never by the explicit-K4 entry points
 * (reloc_pnp_score, reloc_pnp_ransac, reloc_depth_points). */
int reloc_set_distortion(reloc_ctx *ctx, const double *coeffs, int n);
int reloc_get_distortion(reloc_ctx *ctx, double coeffs[5]);
/* cv2.undistortPoints(img, K, dist) without R / P: m pixels (x, y) -> m normalized points (x, y) in double, five
 * fixed-point iterations.  dist = k1 k2 p1 p2 k3 (NULL: zeros). */
int reloc_undistort_points(reloc_ctx *ctx, const float *img, int m, const double K4[4], const double dist[5],
                           double *out_norm);
/* reloc_pnp_score / reloc_pnp_ransac through the distortion model dist = k1 k2 p1 p2 k3 (NULL or all zero: the pinhole
 * entry points' kernels, bit-identical results). */
int reloc_pnp_score_dist(reloc_ctx *ctx, const float *obj, const float *img, int m, const double *Rt, int H,
                         const double K4[4], const double dist[5], float thr_px, int32_t *inlier_count, uint8_t *mask);
int reloc_pnp_ransac_dist(reloc_ctx *ctx, const float *obj, const float *img, int m, const double K4[4],
                          const double dist[5], int iters, float thr_px, double conf, uint64_t seed, double rvec[3],
                          double tvec[3], int32_t *inliers, int32_t *n_inl, int32_t *ok);

/* ---- CLAHE (include/reloc_spec.h, "CLAHE") ------------------------------------------------------- */
/* cv2.createCLAHE(clipLimit, tileGridSize=(tiles_x, tiles_y)).apply(gray) in front of ORB on 3-channel frames.
 * tiles_x == tiles_y == 0 turns it off (the default of a new context; the launch sequence is then that of a context that
 * never had it).  Otherwise both are in 1..64 and clip_limit is finite (<= 0: no clipping), else RELOC_E_ARG.  The first
 * enable allocates the context's CLAHE plane and LUTs.  Applied by reloc_tick, reloc_tick_dev, reloc_tick_batch_dev,
 * reloc_tick_scan_dev, reloc_shard_scan_batch_dev, reloc_record_frame and reloc_orb_frame_dev (the accumulation uses the
 * tick's features); never by reloc_orb_detect_compute or reloc_gray_u8.  Batched calls refuse contexts with unequal
 * settings (RELOC_E_STATE).  reloc_get_clahe returns (0, 0, 0) when off. */
int reloc_set_clahe(reloc_ctx *ctx, double clip_limit, int tiles_x, int tiles_y);
int reloc_get_clahe(reloc_ctx *ctx, double *clip_limit, int32_t *tiles_x, int32_t *tiles_y);
/* The same operation on a caller's gray image with explicit parameters (cv2 shim): any w, h >= 1 within the capacity,
 * tiles in 1..64; out is w x h, dense.  Host pointers; synchronous. */
int reloc_clahe_u8(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride, double clip_limit, int tiles_x,
                   int tiles_y, uint8_t *out);

/* ---- rectification (include/reloc_spec.h, "REMAP") ------------------------------------------------ */
/* cv2.remap(gray, map1, map2, INTER_LINEAR) with BORDER_CONSTANT 0 in front of ORB (and of CLAHE) on 3-channel frames, with
 * the map in OpenCV's fixed-point form: xy = int16[h][w][2] (CV_16SC2), alpha = uint16[h][w] (CV_16UC1), as
 * cv2.convertMaps / cv2.initUndistortRectifyMap(..., CV_16SC2) hand them back.  Host pointers, copied into memory the context
 * owns (allocated on the first enable).  xy == NULL turns it off (the default of a new context; the launch sequence is then
 * that of a context that never had a map).  w, h within the context's capacity (RELOC_E_CAPACITY); every frame passed later
 * must be exactly w x h, else RELOC_E_ARG.  Applied by the entry points that apply CLAHE, before it: frame -> gray + remap ->
 * [CLAHE] -> ORB.  reloc_record_frame and reloc_tick_accumulate_dev also read the depth through the map
 * (cv2.remap(depth, xy, alpha, INTER_NEAREST), border 0 = no depth).  Never applied by reloc_orb_detect_compute,
 * reloc_gray_u8 or reloc_clahe_u8.  Batched calls refuse contexts that are not all on with one map size or all off
 * (RELOC_E_STATE); the map contents may differ per context (a stereo pair).  Independent of reloc_set_camera and
 * reloc_set_distortion: a rectified camera is normally a pinhole with the newCameraMatrix the map was built for, and it is
 * the caller who sets that matrix and leaves the distortion empty.  reloc_get_rectify_map returns (0, 0) when off. */
int reloc_set_rectify_map(reloc_ctx *ctx, const int16_t *xy, const uint16_t *alpha, int w, int h);
int reloc_get_rectify_map(reloc_ctx *ctx, int32_t *w, int32_t *h);
/* cv2.remap on a caller's image (cv2 shim): src is sw x sh with 1 or 3 interleaved channels, the map and out are dw x dh,
 * dense; any sizes >= 1 within the capacity.  nearest = 0: INTER_LINEAR; nearest = 1: INTER_NEAREST (the pixel at xy; alpha
 * may be NULL).  BORDER_CONSTANT with border_value in every channel.  reloc_remap_u16: single channel, nearest only (depth).
 * sstride in bytes.  Host pointers; synchronous. */
int reloc_remap_u8(reloc_ctx *ctx, const uint8_t *src, int sw, int sh, int sstride, int channels, const int16_t *xy,
                   const uint16_t *alpha, int dw, int dh, int nearest, int border_value, uint8_t *out);
int reloc_remap_u16(reloc_ctx *ctx, const uint16_t *src, int sw, int sh, int sstride, const int16_t *xy, int dw, int dh,
                    int border_value, uint16_t *out);
/* cv2.convertMaps(mapx, mapy, CV_16SC2, nninterpolation): float32 w x h maps to the fixed-point pair; with nninterpolation
 * xy is the rounded coordinate and alpha is 0.  Host pointers; synchronous. */
int reloc_convert_maps(reloc_ctx *ctx, const float *mapx, const float *mapy, int w, int h, int nninterpolation,
                       int16_t *xy_out, uint16_t *alpha_out);

/* ---- resize (include/reloc_spec.h, "RESIZE") ------------------------------------------------------- */
/* cv2.resize on a caller's image (cv2 shim): src is sw x sh with 1 or 3 interleaved channels, out is dw x dh, dense; any sizes
 * >= 1 within the capacity (RELOC_E_CAPACITY).  inv_scale_x / inv_scale_y are OpenCV's fx / fy of the call without dsize (the
 * caller computes dw = cvRound(sw * fx) and passes fx on); 0 = dw / sw, the dsize form.  interpolation takes OpenCV's values:
 * 0 INTER_NEAREST, 1 INTER_LINEAR (at exactly 2x on both axes computed as INTER_AREA, as OpenCV does), 3 INTER_AREA (downscale
 * on both axes only); everything else is RELOC_E_ARG.  reloc_resize_u16: single channel, nearest only (depth).  sstride in
 * bytes.  Host pointers; synchronous. */
int reloc_resize_u8(reloc_ctx *ctx, const uint8_t *src, int sw, int sh, int sstride, int channels, uint8_t *out, int dw, int dh,
                    double inv_scale_x, double inv_scale_y, int interpolation);
int reloc_resize_u16(reloc_ctx *ctx, const uint16_t *src, int sw, int sh, int sstride, uint16_t *out, int dw, int dh,
                     double inv_scale_x, double inv_scale_y);
/* The downscale stage at the head of the image chain: cv2.resize(gray, (dw, dh), interpolation=INTER_AREA) of every
 * 3-channel frame, so the chain is frame -> gray + resize -> [rectify] -> [CLAHE] -> ORB.  1 <= dw <= sw, 1 <= dh <= sh
 * (RELOC_E_ARG) and sw x sh within the context's capacity (RELOC_E_CAPACITY): the context is created for the camera's size.
 * (0, 0, 0, 0) turns it off (the default of a new context; the launch sequence is then that of a context that never had it).
 * Applied by the entry points that apply the rectification map.  Every frame passed later must be exactly sw x sh, else
 * RELOC_E_ARG; from the resize on, the working frame is dw x dh (at least 64 x 64 for ORB): it is the size of the rectification
 * map, of CLAHE's grid and the pyramid, of the recorder's border gates, of keypoint and result coordinates, and of the camera
 * (reloc_set_camera takes the intrinsics of the working image: fx' = fx / s, cx' = (cx + 0.5) / s - 0.5 for s = sw / dw).
 * reloc_record_frame and reloc_tick_accumulate_dev take the depth at sw x sh and resize it with INTER_NEAREST before the
 * rectification map's nearest read.  Never applied by reloc_orb_detect_compute, reloc_gray_u8, reloc_clahe_u8 or
 * reloc_remap_*.  Batched calls refuse contexts that are not all off or all on with equal sizes (RELOC_E_STATE).
 * reloc_get_resize returns zeros when off. */
int reloc_set_resize(reloc_ctx *ctx, int sw, int sh, int dw, int dh);
int reloc_get_resize(reloc_ctx *ctx, int32_t *sw, int32_t *sh, int32_t *dw, int32_t *dh);

/* ---- Bayer demosaicing (include/reloc_spec.h, "BAYER") -------------------------------------------- */
/* cv2.cvtColor(raw, code) on a caller's 8-bit mosaic (cv2 shim): raw is w x h, single channel, rows stride bytes apart;
 * out_bgr is w x h x 3, interleaved B G R, dense.  code takes OpenCV's values: 46 COLOR_BayerBG2BGR, 47 COLOR_BayerGB2BGR,
 * 48 COLOR_BayerRG2BGR, 49 COLOR_BayerGR2BGR (a 2RGB code is the aliased 2BGR one); anything else, w < 3 or h < 3 is
 * RELOC_E_ARG, a mosaic beyond the context's capacity RELOC_E_CAPACITY.  Host pointers; synchronous. */
int reloc_bayer_u8(reloc_ctx *ctx, const uint8_t *raw, int w, int h, int stride, int code, uint8_t *out_bgr);
/* The raw-sensor stage in front of the whole image chain: with code = 46..49 every entry point that applies the downscale
 * stage takes a SINGLE-CHANNEL w x h mosaic, rows dense (reloc_orb_frame_dev: stride in bytes of the mosaic, >= w), in place
 * of the 3-channel frame, and the chain is raw -> demosaic + gray -> [resize] -> [rectify] -> [CLAHE] -> ORB: the bytes of
 * cvtColor(cvtColor(raw, code), COLOR_BGR2GRAY) with the context's gray_coeff_bits.  The channel-order bit of `order` is
 * ignored.  reloc_set_resize's source size is the mosaic's size.  Depth images are not mosaics and follow their chain
 * unchanged.  0 turns the stage off (the default of a new context; the launch sequence is then that of a context that never
 * had it, results bit-identical); any other code is RELOC_E_ARG.  The first enable allocates the context's plane.  Never
 * applied by reloc_orb_detect_compute, reloc_gray_u8, reloc_clahe_u8, reloc_remap_* or reloc_resize_*.  Batched calls refuse
 * contexts with unequal codes (RELOC_E_STATE).  A code while a pixel format is set (reloc_set_pixel_format) is RELOC_E_STATE.
 * reloc_get_bayer returns 0 when off. */
int reloc_set_bayer(reloc_ctx *ctx, int code);
int reloc_get_bayer(reloc_ctx *ctx, int32_t *code);

/* ---- pixel formats (include/reloc_spec.h, "PIXEL FORMATS") -------------------------------------- */
/* cv2.cvtColor(src, COLOR_BGRA2GRAY | COLOR_RGBA2GRAY | COLOR_YUV2GRAY_YUY2 | COLOR_YUV2GRAY_UYVY) on a caller's packed frame
 * (cv2 shim): src is w x h pixels of fmt = RELOC_FMT_BGRA, _RGBA (4 bytes per pixel; the gray conversion with the context's
 * gray_coeff_bits, alpha ignored), _YUYV or _UYVY (2 bytes per pixel, w even; the Y bytes), rows stride bytes apart; out is
 * w x h, dense.  Any size >= 1 x 1 within the context's capacity (RELOC_E_CAPACITY); another fmt, an odd width in 4:2:2 or
 * a stride below the row is RELOC_E_ARG.  Host pointers; synchronous. */
int reloc_cvt_gray_u8(reloc_ctx *ctx, const uint8_t *src, int w, int h, int stride, int fmt, uint8_t *out);
/* cv2.cvtColor(src, COLOR_YUV2BGR_YUY2 | COLOR_YUV2BGR_UYVY) (order 0) and the 2RGB twins (order RELOC_ORDER_RGB): fmt =
 * RELOC_FMT_YUYV or _UYVY, w even; out is w x h x 3, interleaved, dense.  Errors as above.  Host pointers; synchronous. */
int reloc_yuv422_bgr_u8(reloc_ctx *ctx, const uint8_t *src, int w, int h, int stride, int fmt, int order, uint8_t *out);
/* The pixel format of the frames that enter the image chain: with fmt other than RELOC_FMT_BGR every entry point that applies
 * the downscale stage takes w x h frames of that format, rows dense (reloc_orb_frame_dev: stride in bytes, >= w * bytes per
 * pixel), in place of the 3-channel frame: RELOC_FMT_MONO8 1 byte per pixel, the gray itself (no kernel and no launch is
 * added); _BGRA / _RGBA 4 bytes, _YUYV / _UYVY 2 bytes (w even, else RELOC_E_ARG from the entry point), through one unpack
 * launch at the head of the chain, frame -> unpack -> [resize] -> [rectify] -> [CLAHE] -> ORB: the bytes of reloc_cvt_gray_u8.
 * The channel-order bit of `order` is ignored.  reloc_set_resize's source size is the frame's size; the persistent detection
 * mask applies as to any frame of the chain.  Depth images follow their chain unchanged.  RELOC_FMT_BGR (0) restores the
 * default (the launch sequence is then that of a context that never had a format, results bit-identical); a value outside
 * RELOC_FMT_BGR .. RELOC_FMT_UYVY is RELOC_E_ARG.  The format and the Bayer stage exclude each other: a format other than 0
 * while reloc_set_bayer is on, and reloc_set_bayer with a code while a format is set, are RELOC_E_STATE.  The first enable
 * of a packed format allocates the context's plane, and grows the staging plane of the host-pointer entry points for a
 * 4-byte format.  Never applied by reloc_orb_detect_compute*, reloc_gray_u8, reloc_clahe_u8, reloc_remap_*, reloc_resize_*
 * or reloc_bayer_u8.  Batched calls refuse contexts with unequal formats (RELOC_E_STATE). */
int reloc_set_pixel_format(reloc_ctx *ctx, int fmt);
int reloc_get_pixel_format(reloc_ctx *ctx, int32_t *fmt);

/* ---- sparse stereo depth (include/reloc_spec.h, "STEREO") ----------------------------------------- */
/* Depth at the ORB keypoints from the other eye of a rectified pair, for cameras without a depth sensor: an 11 x 11 SAD
 * search along the row with edge, uniqueness and left-right gates, parabola sub-pixel step, depth = fx * baseline / disparity
 * as uint16 millimetres (0 = no depth).  status per keypoint: 0 ok, 1 border, 2 range, 3 edge, 4 uniqueness, 5 left-right,
 * 6 beyond 65535 mm.
 * reloc_set_stereo keeps the setting on a context (the LEFT eye's); baseline_m == 0 switches it off (the default of a new
 * context; no launch, allocation or event is then added to any entry point).  baseline_m finite and >= 0, min_disparity in
 * 0..1024, num_disparities in 8..256, uniqueness in 0..50, lr_check 0 / 1, else RELOC_E_ARG.  The first enable allocates the
 * context's stereo buffers.  reloc_get_stereo returns baseline_m 0 when off. */
int reloc_set_stereo(reloc_ctx *ctx, double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check);
int reloc_get_stereo(reloc_ctx *ctx, double *baseline_m, int32_t *min_disparity, int32_t *num_disparities, int32_t *uniqueness,
                     int32_t *lr_check);
/* Stateless probe with explicit parameters (like reloc_clahe_u8): two gray planes of w x h (w, h >= 11, within the capacity),
 * rows stride bytes apart, n >= 0 keypoints xy (n x 2 f32), fx > 0, baseline_m > 0.
 * depth_mm, disparity, status hold n entries.  Host pointers; synchronous.  Independent of reloc_set_stereo. */
int reloc_stereo_depth(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride,
                       const float *xy, int n, double fx, double baseline_m, int min_disparity, int num_disparities,
                       int uniqueness, int lr_check, uint16_t *depth_mm, float *disparity, uint8_t *status);
/* reloc_record_frame with the right eye's frame in the depth image's place.  The right eye is a context of its own that
 * carries that eye's image chain (pixel format or Bayer code, resize, its own rectification map, CLAHE): its frame runs
 * through the gray half of the chain only, never ORB, on its own stream, ordered against ctx's stream by events.  right must
 * agree with ctx in everything a batched call compares of the chain (and in capacity, device and gray_coeff_bits), else
 * RELOC_E_STATE.  The left plane is level 0 of ctx's pyramid (the chain's output), fx is the context camera's.  The gates
 * of reloc_record_frame apply to the per-keypoint depth except the 3 x 3 variance gate (reloc_spec.h).  *n_stereo = keypoints
 * with status 0.  RELOC_E_STATE while stereo is off on ctx. */
int reloc_record_frame_stereo(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *img, const uint8_t *img_right, int w, int h,
                              int order, int nfeatures, float *xy, uint8_t *desc, float *pts3d, int32_t *kp_index,
                              int32_t *n_out, int32_t *n_kp, int32_t *n_stereo);
/* reloc_tick_accumulate_dev with the right eye's frame (device pointer, a frame of right's chain, dense rows) in the depth
 * image's place; right as above.  The frame is ordered on ctx's stream, like the depth image of reloc_tick_accumulate_dev (copy
 * it with reloc_h2d on ctx).  Enqueues only: the two streams are ordered by events in both directions, the host never waits. */
int reloc_tick_accumulate_stereo_dev(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *img_right_dev, int w, int h, int order,
                                     const double base_pose[7], int silence_ok);
/* Parity tap: the last stereo pass of the context, per keypoint of the frame's ORB output (*n of them; arrays of max_feat
 * entries, any may be NULL).  Synchronises the context's stream. */
int reloc_stereo_debug(reloc_ctx *ctx, uint16_t *depth_mm, float *disparity, uint8_t *status, int32_t *n);

/* ---- dense stereo depth (include/reloc_spec.h, "STEREO, dense") ----------------------------------- */
/* The same matcher at every integer pixel of the working frame: a depth image for everything that takes one
 * (reloc_depth_points, the depth-image form of reloc_record_frame, a log).  Three planes of the working-frame size with
 * dense rows: depth_mm uint16 (0 = no depth), disparity float32 (0 where status != 0), status uint8 (the seven codes above; an eighth,
 * RELOC_STEREO_SPECKLE, only from a pass with the speckle stage on, below).
 * The plane at (rint x, rint y) is what reloc_stereo_depth returns for keypoint (x, y).  The buffers are taken on the first
 * dense call of a context; a context that never makes one allocates and launches nothing of it.
 * reloc_stereo_depth_image is the dense twin of reloc_stereo_depth: two gray planes of w x h (w, h >= 11, within the
 * capacity, else RELOC_E_CAPACITY), rows stride bytes apart, explicit parameters with the same checks.  disparity and status
 * may be NULL.  Host pointers; synchronous.  Independent of reloc_set_stereo. */
int reloc_stereo_depth_image(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, double fx,
                             double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check,
                             uint16_t *depth_mm, float *disparity, uint8_t *status);
/* A pair of host frames (w, h >= 64) through the gray half of both eyes' image chains, paired as reloc_record_frame_stereo pairs
 * them (right: a context of its own with that eye's chain, its own stream, ordered by events; the same agreement checks), and
 * no ORB; then the dense pass with ctx's reloc_set_stereo setting and the context camera's fx.  RELOC_E_STATE while stereo is
 * off on ctx, RELOC_E_ARG for right == ctx.  The plane stays on the device (reloc_stereo_dense_debug, reloc_stereo_frame_points);
 * depth_mm (working-frame size, may be NULL) receives a copy.  *out_w x *out_h (may be NULL): the working frame.  Synchronous. */
int reloc_stereo_frame_depth(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *img, const uint8_t *img_right, int w, int h,
                             int order, uint16_t *depth_mm, int32_t *out_w, int32_t *out_h);
/* The same pass, then the obstacle cloud of reloc_depth_points from the plane on the device with the context camera's K4:
 * the depth makes no trip through the host.  step > 0; points holds ceil(W/step) * ceil(H/step) rows of 3 floats of the
 * working frame W x H; the output contract is that of reloc_depth_points. */
int reloc_stereo_frame_points(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *img, const uint8_t *img_right, int w, int h,
                              int order, int step, float zmin, float zmax, float *points, int32_t *n_out);
/* Parity tap: the three planes of the context's last dense pass, *w x *h of them (arrays of the context's capacity
 * max_w x max_h, or of the pass's size; any pointer may be NULL).  RELOC_E_STATE before the first pass.  Synchronises the
 * context's stream. */
int reloc_stereo_dense_debug(reloc_ctx *ctx, uint16_t *depth_mm, float *disparity, uint8_t *status, int32_t *w, int32_t *h);

/* ---- semi-global aggregation (include/reloc_spec.h, "STEREO, semi-global") ------------------------- */
/* The dense pass with the SAD costs aggregated along 4 or 8 directions before the selection; this project's own matcher, not
 * OpenCV's StereoSGBM.  A persistent setting of the LEFT context: paths 0 = off (a new context; p1, p2 are then ignored and
 * return to their defaults), 4 (mask 0x0F) or 8 (mask 0xFF); 0 <= p1 <= p2 <= RELOC_STEREO_SGM_P2_MAX.  Independent of
 * reloc_set_stereo and of reloc_set_stereo_speckle.  It applies to every dense pass that runs with the context's settings
 * (reloc_stereo_frame_depth, reloc_stereo_frame_points, and so to what reloc_occ_integrate_stereo_dev,
 * reloc_corr_match_stereo_dev, reloc_obs_*_stereo_dev and reloc_stereo_dense_debug read).  Bad values return RELOC_E_ARG and
 * change nothing.  The volumes (6 bytes per pixel and disparity) are taken at the first semi-global pass and sized from it;
 * RELOC_E_CAPACITY when the device has no room for them, the context stays usable. */
int reloc_set_stereo_sgm(reloc_ctx *ctx, int paths, int p1, int p2);
int reloc_get_stereo_sgm(reloc_ctx *ctx, int32_t *paths, int32_t *p1, int32_t *p2);
/* The explicit twin of reloc_stereo_depth_image, with the same checks: path_mask in 1..255 (bit b selects direction b of the
 * specification), the penalties as above.  Never speckle-filtered.  Host pointers; synchronous. */
int reloc_stereo_sgm_image(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, double fx,
                           double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check,
                           int path_mask, int p1, int p2, uint16_t *depth_mm, float *disparity, uint8_t *status);
/* Parity tap: the sum volume S of the context's last semi-global pass as [v][u][k], k = d - min_disparity, *w * *h * *nd
 * values, 0xFFFFFFFF at undefined entries.  S may be NULL (the sizes only).  RELOC_E_STATE before the first such pass.  With
 * reloc_stereo_sgm_image and a single-bit mask it is the per-direction tap. */
int reloc_stereo_sgm_debug(reloc_ctx *ctx, uint32_t *S, int32_t *w, int32_t *h, int32_t *nd);

/* ---- census cost (include/reloc_spec.h, "STEREO, census") ------------------------------------------ */
/* The data term of the three matchers: RELOC_STEREO_COST_SAD (0, a new context) or RELOC_STEREO_COST_CENSUS (1), the Hamming
 * distance of 8-bit census transforms of both eyes, for pairs that are exposed unequally.  A persistent setting of the LEFT
 * context, independent of reloc_set_stereo, reloc_set_stereo_speckle and reloc_set_stereo_sgm.  It applies to every pass
 * that runs with the context's settings (reloc_record_frame_stereo, reloc_tick_accumulate_stereo_dev,
 * reloc_stereo_frame_depth, reloc_stereo_frame_points, and so to what reloc_occ_integrate_stereo_dev,
 * reloc_corr_match_stereo_dev, reloc_obs_*_stereo_dev, reloc_stereo_debug and reloc_stereo_dense_debug read).  A value
 * outside 0..1 returns RELOC_E_ARG and changes nothing.  The two census planes (2 bytes per pixel of the capacity) are taken
 * on the first census pass; a context that never selects the census allocates and launches nothing of it. */
int reloc_set_stereo_cost(reloc_ctx *ctx, int cost);
int reloc_get_stereo_cost(reloc_ctx *ctx, int32_t *cost);
/* reloc_stereo_depth with the cost as a parameter (reloc_stereo_depth itself means cost 0); the same checks. */
int reloc_stereo_depth_cost(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride,
                            const float *xy, int n, double fx, double baseline_m, int min_disparity, int num_disparities,
                            int uniqueness, int lr_check, int cost, uint16_t *depth_mm, float *disparity, uint8_t *status);
/* reloc_stereo_sgm_image with the cost as a parameter; path_mask 0 means no aggregation (reloc_stereo_depth_image with that
 * cost; p1, p2 are then ignored).  reloc_stereo_depth_image and reloc_stereo_sgm_image themselves mean cost 0. */
int reloc_stereo_image_cost(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, double fx,
                            double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check, int cost,
                            int path_mask, int p1, int p2, uint16_t *depth_mm, float *disparity, uint8_t *status);
/* Parity tap: the census transform alone of a gray plane of w x h (w, h >= 1, within the capacity), rows stride >= w bytes
 * apart, into out (w x h, dense rows).  No byte of the padding is read.  Host pointers; synchronous. */
int reloc_census(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride, uint8_t *out);

/* ---- speckle filter (include/reloc_spec.h, "STEREO, speckle") -------------------------------------- */
/* OpenCV's filterSpeckles on an int16 plane of w x h, rows stride ELEMENTS apart, in place: every pixel of a 4-connected
 * component (valid = differs from new_val; joined = |a - b| <= max_diff) of at most max_speckle_size pixels becomes new_val;
 * the padding of a row is neither read nor written.  Host pointer; synchronous.  RELOC_E_ARG for w or h < 1, stride < w, a
 * negative limit or a new_val outside int16; RELOC_E_CAPACITY beyond the context's max_w x max_h. */
int reloc_filter_speckles(reloc_ctx *ctx, int16_t *img, int w, int h, int stride, int new_val, int max_speckle_size, int max_diff);
/* The speckle stage of the dense pass, a persistent setting of the LEFT context: window = the component size limit in pixels,
 * 0 = off (a new context); range in whole disparities, 0..RELOC_STEREO_SPECKLE_RANGE_MAX.  Independent of reloc_set_stereo.
 * It applies to every dense pass that runs with the context's settings (reloc_stereo_frame_depth, reloc_stereo_frame_points,
 * and so to what reloc_occ_integrate_stereo_dev, reloc_corr_match_stereo_dev and reloc_stereo_dense_debug read): a removed
 * pixel has status RELOC_STEREO_SPECKLE, depth_mm 0 and disparity 0.  reloc_stereo_depth_image takes its parameters
 * explicitly and is never filtered.  With window 0 a pass launches what it always launched. */
int reloc_set_stereo_speckle(reloc_ctx *ctx, int window, int range);
int reloc_get_stereo_speckle(reloc_ctx *ctx, int32_t *window, int32_t *range);

/* ---- teach-time occupancy map (include/reloc_spec.h, "OCCUPANCY") ---------------------------------- */
/* The log-odds grid of the reference's teach_run_depth_mapper.py: every frame's obstacle cloud is taken into the map frame,
 * height-filtered, subsampled and ray-traced from the sensor's cell into a grid of int8 units of 0.2 (free -2, hit +7, bounds
 * -25 / +25, one clamped update per cell per frame).  T12: the 3 x 4 sensor-to-map transform, row major, finite.  out_rays
 * (may be NULL): the rays of the frame, what total_points_integrated grew by.
 * reloc_occ_configure allocates and zeroes a grid of w_cells x h_cells cells of res metres with cell (0, 0) at (origin_x,
 * origin_y), counters included; a second call resets it.  Non-positive sizes, res or subsample, anything not finite:
 * RELOC_E_ARG; more than RELOC_OCC_MAX_CELLS cells or 32768 per side: RELOC_E_CAPACITY.  A context that never configures a
 * map allocates and launches nothing of it.  Every integrate entry point and reloc_occ_read return RELOC_E_STATE before it. */
int reloc_occ_configure(reloc_ctx *ctx, double origin_x, double origin_y, double res, int w_cells, int h_cells, double z_lo,
                        double z_hi, int subsample);
/* A host cloud of n >= 0 rows of 3 floats in any sensor frame (pts may be NULL when n == 0).  Synchronous. */
int reloc_occ_integrate_points(reloc_ctx *ctx, const float *pts, int n, const double T12[12], int32_t *out_rays);
/* A host depth image as reloc_depth_points takes it, through that cloud, which is never written.  Synchronous. */
int reloc_occ_integrate_depth(reloc_ctx *ctx, const void *depth, int is_f32, int w, int h, int step, const double K4[4],
                              float zmin, float zmax, const double T12[12], int32_t *out_rays);
/* The depth plane of the context's last dense stereo pass where it lies on the device, with the context camera's K4: the
 * cloud of reloc_stereo_frame_points.  RELOC_E_STATE before the first pass.  With out_rays == NULL it enqueues only. */
int reloc_occ_integrate_stereo_dev(reloc_ctx *ctx, int step, float zmin, float zmax, const double T12[12], int32_t *out_rays);
/* units: h_cells x w_cells int8, row 0 at origin_y.  pgm: the same size, 0 occupied (units >= 4) / 254 free (units <= -6) / 205
 * unknown, rows flipped.  counters: frames_integrated, total_points_integrated, frames_skipped_empty.  Any pointer may be
 * NULL.  Synchronous. */
int reloc_occ_read(reloc_ctx *ctx, int8_t *units, uint8_t *pgm, int64_t counters[3]);

/* ---- depth-correlation anchor (include/reloc_spec.h, "CORRELATION") ------------------------------- */
/* The second anchor channel of the reference's depth_correlation_matcher.py: the cells of the current depth cloud slid over the
 * dilated teach occupancy map, hits counted at every offset of a table, best and second best picked on the device.
 * reloc_corr_set_map takes the occupied plane (h x w uint8, row 0 at origin_y, non-zero = occupied; cell (0, 0) at (origin_x,
 * origin_y), res metres per cell), packs it to one bit per cell and dilates it `dilate` times by the 4-connected cross.  A
 * second call replaces the map.  reloc_corr_set_map_from_occ takes the context's live occupancy grid (units >= 4, its
 * geometry) where it lies: RELOC_E_STATE without one.  Non-positive sizes or res, dilate < 0, anything not finite: RELOC_E_ARG;
 * more than RELOC_CORR_MAX_CELLS cells, RELOC_CORR_MAX_SIDE per side or RELOC_CORR_MAX_DILATE iterations, or a cell size under
 * which the configured max_range no longer fits the window: RELOC_E_CAPACITY, the map before stays.  A context that never sets
 * a map allocates and launches nothing of this.  Every other entry point here returns RELOC_E_STATE before a map is set. */
int reloc_corr_set_map(reloc_ctx *ctx, const uint8_t *occupied, int w, int h, double origin_x, double origin_y, double res,
                       int dilate);
int reloc_corr_set_map_from_occ(reloc_ctx *ctx, int dilate);
/* The search: cell_offsets, the n_side = 2 ns + 1 cell offsets of rule (g), index i for columns and j for rows; the height
 * band, the range about the base position and the least number of points (rules (d), (e)).  n_side even or < 1, min_points
 * < 0, max_range <= 0, anything not finite: RELOC_E_ARG.  n_side > RELOC_CORR_MAX_TABLE, an offset beyond
 * RELOC_CORR_MAX_OFFSET cells, or 2 * (ceil(max_range / res) + 2) + 1 > RELOC_CORR_MAX_WINDOW: RELOC_E_CAPACITY. */
int reloc_corr_configure(reloc_ctx *ctx, const int32_t *cell_offsets, int n_side, double z_lo, double z_hi, double max_range,
                         int min_points);
/* One tick from each of the occupancy map's three sources (reloc_occ_integrate_*): T12 the 3 x 4 sensor-to-map transform,
 * (vio_x, vio_y) the base position, all finite (RELOC_E_ARG).  record: RELOC_CORR_RECORD_WORDS int32 -- status RELOC_CORR_*,
 * kept points, points in the map, n_cells, best i, best j (in [-ns, ns]), best hits, second hits.  surface (may be NULL):
 * n_side x n_side int32 hits, [i + ns][j + ns]; all zero behind a status other than RELOC_CORR_OK.  RELOC_E_STATE before
 * reloc_corr_configure.  Synchronous. */
int reloc_corr_match_points(reloc_ctx *ctx, const float *pts, int n, const double T12[12], double vio_x, double vio_y,
                            int32_t *record, int32_t *surface);
int reloc_corr_match_depth(reloc_ctx *ctx, const void *depth, int is_f32, int w, int h, int step, const double K4[4], float zmin,
                           float zmax, const double T12[12], double vio_x, double vio_y, int32_t *record, int32_t *surface);
int reloc_corr_match_stereo_dev(reloc_ctx *ctx, int step, float zmin, float zmax, const double T12[12], double vio_x, double vio_y,
                                int32_t *record, int32_t *surface);
/* The dilated map unpacked: h x w uint8 of 0 / 1, row 0 at origin_y (plane may be NULL); *w, *h: its size (may be NULL). */
int reloc_corr_read_map(reloc_ctx *ctx, uint8_t *plane, int32_t *w, int32_t *h);

/* ---- route clearance (include/reloc_spec.h, "ROUTE") --------------------------------------------- */
/* What the reference's sanitize_route.py and send_goals_hybrid.py walk a grid for: the distance from a cell to the nearest
 * occupied one, and the first cell of the walk's order that satisfies a predicate.  All synchronous.
 * reloc_route_set_map takes the occupied plane (h x w uint8, row 0 at origin_y, non-zero = occupied), ORs in n_stamps rectangles
 * (n_stamps x 4 int32: r_lo, r_hi, c_lo, c_hi, half open, clipped to the plane) and computes the clearance plane of rule (d)
 * with `cap`; row_remap (h int32) and col_remap (w int32) are the tables of rule (e), NULL = identity.  A second call replaces
 * the map.  reloc_route_set_map_from_occ takes the context's live occupancy grid (units >= 4) where it lies: RELOC_E_STATE
 * without one.  Non-positive sizes, cap outside [0, 254], a remap entry outside the plane, a stamp with lo > hi: RELOC_E_ARG;
 * more than RELOC_OCC_MAX_CELLS cells or RELOC_ROUTE_MAX_SIDE per side: RELOC_E_CAPACITY; the map before stays in both cases.  A
 * context that never sets a route map or a costmap allocates and launches nothing of this. */
int reloc_route_set_map(reloc_ctx *ctx, const uint8_t *occupied, int w, int h, const int32_t *stamps, int n_stamps, int cap,
                        const int32_t *row_remap, const int32_t *col_remap);
int reloc_route_set_map_from_occ(reloc_ctx *ctx, const int32_t *stamps, int n_stamps, int cap, const int32_t *row_remap,
                                 const int32_t *col_remap);
/* The clearance plane: h x w uint8, row 0 at origin_y (plane may be NULL); *w, *h: its size (may be NULL).  RELOC_E_STATE
 * before a map is set, as reloc_route_clearance_at. */
int reloc_route_read_clearance(reloc_ctx *ctx, uint8_t *plane, int32_t *w, int32_t *h);
/* out[i] = the clearance at cell (cells_rc[2 i], cells_rc[2 i + 1]) = (row, col), no remap; RELOC_ROUTE_FAR for a cell outside
 * the plane.  n == 0 launches nothing. */
int reloc_route_clearance_at(reloc_ctx *ctx, const int32_t *cells_rc, int n, uint8_t *out);
/* The int8 costmap of the COST predicate (h x w, row 0 at its origin_y), a plane of its own beside the route map; a second call
 * replaces it.  Capacity as the map's. */
int reloc_route_set_costmap(reloc_ctx *ctx, const int8_t *cost, int w, int h);
/* Rule (g): offsets_rc is the order table (n_offsets x 2 int32: dr, dc), cells_rc the n start cells (row, col; any int32);
 * out_index[i] = the first table index whose cell is inside the plane and satisfies the predicate, -1 for none.
 * RELOC_ROUTE_PRED_CLEARANCE: clearance at the remapped cell >= thresh, RELOC_E_STATE before a route map;
 * RELOC_ROUTE_PRED_COST: 0 <= cost < thresh, RELOC_E_STATE before a costmap.  Another predicate: RELOC_E_ARG.  More than
 * RELOC_ROUTE_MAX_OFFSETS entries, or one beyond RELOC_ROUTE_MAX_OFFSET cells: RELOC_E_CAPACITY.  n == 0 launches nothing. */
int reloc_route_search(reloc_ctx *ctx, int predicate, int thresh, const int32_t *offsets_rc, int n_offsets, const int32_t *cells_rc,
                       int n, int32_t *out_index);

/* ---- local obstacles (include/reloc_spec.h, "OBSTACLE") ------------------------------------------ */
/* What the reference's traversability_filter.py, gap_navigator.py (its depth profile) and local_obstacle_grid.py compute of every
 * depth frame.  A depth image is h x w float32 (metres) or uint16 (millimetres) in host memory, w <= RELOC_OBS_MAX_COLS and
 * w * h within the context's capacity (RELOC_E_CAPACITY), or the plane the context's last dense stereo pass left on the device
 * (*_stereo_dev: RELOC_E_STATE before the first pass).  A context that never calls any of this allocates and launches nothing
 * of it.  A refused call leaves the filter, the grid and its configuration as they were.
 * reloc_obs_set_filter: the traversability filter of rule (d); bh == 0 && bw == 0 switches it off (the default), otherwise sides
 * in [RELOC_OBS_MIN_BLOCK, RELOC_OBS_MAX_BLOCK] (RELOC_E_CAPACITY), 0 <= lo < hi, min_count >= 1, coverage > 0, everything
 * finite (RELOC_E_ARG).  The getter also returns n_cov. */
int reloc_obs_set_filter(reloc_ctx *ctx, int bh, int bw, float lo, float hi, int min_count, double coverage, double var_thresh,
                         double min_solid, float fill);
int reloc_obs_get_filter(reloc_ctx *ctx, int32_t *bh, int32_t *bw, float *lo, float *hi, int32_t *min_count, int32_t *n_cov,
                         double *var_thresh, double *min_solid, float *fill);
/* The filter on one host image: filtered (h x w float32 metres, may be NULL) and mask ((h / bh) x (w / bw) bytes, 1 =
 * traversable, may be NULL).  RELOC_E_STATE while the filter is off.  Synchronous. */
int reloc_obs_filter_depth(reloc_ctx *ctx, const void *depth, int is_f32, int w, int h, float *filtered, uint8_t *mask);
/* Rules (a)-(c): profile and counts take ceil(w / step) entries each (either may be NULL).  use_filter != 0: the pixels are
 * those of the filtered image (RELOC_E_STATE while the filter is off).  step >= 1, 0 <= lo, q in [0, 100], min_valid >= 1,
 * everything finite (RELOC_E_ARG); a strip of more than RELOC_OBS_MAX_STRIP rows: RELOC_E_CAPACITY.  Synchronous; the
 * _stereo_dev form with both outputs NULL enqueues only. */
int reloc_obs_profile_depth(reloc_ctx *ctx, const void *depth, int is_f32, int w, int h, int step, float lo, float hi, int q,
                            int min_valid, float fill, int use_filter, float *profile, int32_t *counts);
int reloc_obs_profile_stereo_dev(reloc_ctx *ctx, int step, float lo, float hi, int q, int min_valid, float fill, int use_filter,
                                 float *profile, int32_t *counts);
/* The ego grid of rule (e): cells x cells zeros, and what every update projects with: the profile's parameters as above.
 * cells in [1, RELOC_OBS_MAX_CELLS] (RELOC_E_CAPACITY); res, decay, hit, hit_nb, obstacle_hits positive and finite
 * (RELOC_E_ARG).  A second call resets the grid.  Everything below returns RELOC_E_STATE before it. */
int reloc_obs_grid_configure(reloc_ctx *ctx, int cells, double res, float decay, float hit, float hit_nb, float obstacle_hits,
                             int step, float lo, float hi, int q, int min_valid, int use_filter);
/* One update: shift by (sx, sy) cells, decay, and with depth != NULL the projection along dirs: ceil(w / step) pairs (c, s) of
 * float64, n_dirs of them (another count: RELOC_E_ARG; more than RELOC_OBS_MAX_GRID_COLS: RELOC_E_CAPACITY).  depth == NULL:
 * shift and decay only, the other arguments are ignored.  Synchronous; the _stereo_dev form enqueues only. */
int reloc_obs_grid_update_depth(reloc_ctx *ctx, int sx, int sy, const void *depth, int is_f32, int w, int h, const double *dirs,
                                int n_dirs);
int reloc_obs_grid_update_stereo_dev(reloc_ctx *ctx, int sx, int sy, const double *dirs, int n_dirs);
/* Rule (f): n sectors along dirs (n pairs (c, s)), out n float64.  max_range finite; n > RELOC_OBS_MAX_SECTORS or
 * max_range / res > RELOC_OBS_MAX_STEPS: RELOC_E_CAPACITY.  n == 0 launches nothing. */
int reloc_obs_grid_profile(reloc_ctx *ctx, const double *dirs, int n, double max_range, double *out);
/* Rule (g): grid cells x cells float32, image the same size uint8, the count of cells >= obstacle_hits and the maximum; any
 * pointer may be NULL.  *cells: the side (may be NULL). */
int reloc_obs_grid_read(reloc_ctx *ctx, float *grid, uint8_t *image, int32_t *obstacle_cells, float *max_hits, int32_t *cells);

/* cv2.erode / cv2.dilate of an 8-bit single-channel image (rows `stride` bytes apart) with a kh x kw all-ones rectangle anchored
 * at (kw / 2, kh / 2), `iterations` times, OpenCV's default border: a pixel outside the image never lowers an erosion and never
 * raises a dilation.  dst: dense rows of w.  dilate: 0 erode, 1 dilate.  A side beyond RELOC_MORPH_MAX_KERNEL, more than
 * RELOC_MORPH_MAX_ITERATIONS or an image beyond the context's capacity: RELOC_E_CAPACITY.  Synchronous. */
int reloc_morph_rect(reloc_ctx *ctx, const uint8_t *src, int w, int h, int stride, int kw, int kh, int dilate, int iterations,
                     uint8_t *dst);

/* ---- fused tick ----------------------------------------------------------------------------- */
#define RELOC_TICK_LOCAL   0   /* candidates by VIO distance / heading only                          M:293-302 */
#define RELOC_TICK_GLOBAL  1   /* whole-database search unconditionally (the benchmarked shape)       G:329-344 */
#define RELOC_TICK_AUTO    2   /* local first; whole-database search only if it finds no candidate -- the host passes
                                  this mode when G's silence and drift conditions hold                G:324-326 */
/* One repeat tick against the selected database (M:281-433 with G:315-344's whole-database
 * candidate search according to global_reloc = RELOC_TICK_*): gray -> ORB -> candidates -> mutual match ->
 * PnP-RANSAC -> reprojection gate -> pose compose -> best by inliers -> consistency gate.
 * base_pose: x y z qx qy qz qw of base_link (the /tmp/isaac_pose.txt line).
 * Outputs: anchor_pose[7] (base_link in the teach map), n_inl, reproj (px), lm_idx, outcome,
 * n_candidates.  Host pointers; synchronous. */
int reloc_tick(reloc_ctx *ctx, const uint8_t *img, int w, int h, int order, const double base_pose[7],
               int global_reloc, uint64_t seed, double anchor_pose[7], int32_t *n_inl, float *reproj,
               int32_t *lm_idx, int32_t *outcome, int32_t *n_candidates);
/* Same with the frame already resident in device memory; enqueues everything and leaves the
 * result in a ctx-owned device record readable with reloc_tick_result(). */
int reloc_tick_dev(reloc_ctx *ctx, const uint8_t *img_dev, int w, int h, int order,
                   const double base_pose[7], int global_reloc, uint64_t seed);
/* Batched relocalization (BASELINE.json config 4): n <= 8 frames, one context per frame; the contexts share ONE stream
 * (reloc_set_stream), one device and one database (reloc_db_share).  ORB of every frame, then ONE launch that scans the
 * database for all n frames (the launch-fixed cost of the scan is paid once per batch), then ranking / matches / PnP /
 * gates per frame.  Results per context as after reloc_tick_dev.  base_poses: n x 7, seeds: n or NULL. */
int reloc_tick_batch_dev(reloc_ctx *const *ctxs, int n, const uint8_t *const *imgs_dev, int w, int h, int order,
                         const double *base_poses, int global_reloc, const uint64_t *seeds);
/* The result of the last tick enqueued on ctx.  WAITS FOR THAT TICK'S RECORD ONLY (reloc_tick_wait below), not for the stream:
 * since round 3 this call is no stream barrier -- work enqueued behind the tick (reloc_tick_accumulate_dev, copies, the scan half
 * of a next frame) may still be running when it returns; call reloc_sync() before touching anything such work writes.  If the
 * last tick entry point on ctx returned an error before its result record was enqueued, this returns RELOC_E_STATE (it never
 * hands out the previous tick's record in its place). */
int reloc_tick_result(reloc_ctx *ctx, double anchor_pose[7], int32_t *n_inl, float *reproj,
                      int32_t *lm_idx, int32_t *outcome, int32_t *n_candidates);
/* Waits for the result record of the last tick enqueued on ctx -- and only for that: the tick's last kernel stores the
 * record into pinned host memory and, behind it, a sequence stamp; this call polls the stamp instead of going through the
 * stream-completion path of the runtime (10-50 us cheaper per synchronous tick, most after an idle period).  Falls back to
 * a stream synchronisation after 20 ms.  reloc_tick_result() / reloc_tick_result_ex() wait this way themselves. */
int reloc_tick_wait(reloc_ctx *ctx);
/* Device address of the 96-byte result record of the last tick (layout of reloc_tick_result_ex's outputs: double
 * anchor_pose[7], double reproj, int32 n_inl, lm_idx, outcome, n_candidates, n_features, relocating): lets a pipelined
 * host copy results with reloc_d2h into pinned memory without synchronising per frame.
 * Every outcome writes all 96 bytes.  The three outcomes without a pose (NO_FEATURES, NO_CANDIDATES, NO_PNP_ACCEPT) leave
 * anchor_pose all zero, reproj 0, n_inl 0 and lm_idx -1; CONSISTENCY_FAIL keeps anchor_pose, reproj, n_inl and lm_idx of the
 * rejected anchor.  n_candidates (also under NO_FEATURES: the candidates were still found), n_features and relocating are
 * reported by all five.  Word 22 is 0 in the device record (the sequence stamp goes to host records only), word 23 is 0
 * (tests/test_gpu_finalize.py). */
const void *reloc_tick_result_dev(reloc_ctx *ctx);
/* Streaming without a copy: the ticks enqueued after this call ALSO write their 96-byte result record (same layout) to
 * `pinned_record`, memory from reloc_host_alloc() -- the last kernel of the tick stores it over PCIe itself, so the record
 * is complete once the ctx stream has passed that tick (event / reloc_sync) -- or as soon as its int32 word 22 (byte 88)
 * holds the tick's sequence stamp, which the kernel stores last, system-scope release.  Point it at a different record before each
 * tick to keep one per frame; NULL stops it.  (reloc_tick_result() reads an internal record of the same kind.) */
int reloc_tick_result_to(reloc_ctx *ctx, void *pinned_record);
/* Deployment hint, no effect on results: `on` > 0 says this context is the only stream of work on the GPU (one robot,
 * one camera).  The whole-database scan then runs as ONE resident generation of workgroups (no early hand-over of CU
 * slots to other streams' kernels) and the tick's small kernels take the shapes that are fastest alone (8 waves per
 * record in the emit pass, full register set in the PnP refinement): ~12 us less per synchronous global tick, at the
 * price of ~10 % throughput if several such contexts do run side by side.  `on` == 0: it is not alone.  `on` < 0 (the
 * default): decided per call -- alone while it is the only live context this process has created with reloc_create. */
int reloc_set_exclusive(reloc_ctx *ctx, int on);
/* Same plus n_features and the `relocating` flag (1 when the whole-database search produced the candidates, G:344); waits like
 * reloc_tick_result (the tick's record only; RELOC_E_STATE after a tick that failed to enqueue). */
int reloc_tick_result_ex(reloc_ctx *ctx, double anchor_pose[7], int32_t *n_inl, double *reproj, int32_t *lm_idx,
                         int32_t *outcome, int32_t *n_candidates, int32_t *n_features, int32_t *relocating);
/* Accumulation (M:435-500), enqueued behind a tick on the same ctx: when the tick's outcome is no_candidates /
 * no_pnp_accept / consistency_fail (M:314,384,396), silence_ok is set (the host's `ts - last_anchor_ts >=
 * ACCUM_SILENCE_S`, M:441) and no record is filed within accum_min_dist_m of the robot, the current frame's keypoints
 * with valid depth become a new record at the tail of the arena (>= accum_min_kpts of them).  depth_mm_dev: (h, w)
 * uint16 millimetres in device memory.  The arena must have room for one record of max_feat rows (reloc_db_reserve);
 * reloc_accumulate_result() synchronises, reports what happened and makes the new record visible to later ticks. */
int reloc_tick_accumulate_dev(reloc_ctx *ctx, const uint16_t *depth_mm_dev, int w, int h, const double base_pose[7],
                              int silence_ok);
int reloc_accumulate_result(reloc_ctx *ctx, int32_t *appended, int32_t *n_kpts, double *nearest_m);
/* Parity tap: per-candidate records of the last tick (arrays of 32 entries; Rt 32 x 12).  Three shapes, by what the tick's inlier
 * gate (min_inliers; global_min_inliers in a whole-database search) lets a candidate become:
 *   consensus set >= gate         refined: ok 1, n_inl, the refined pose, reproj = mean reprojection error of the inliers
 *   matches >= gate > consensus   cannot be accepted, not refined: ok as RANSAC left it, n_inl = the consensus size, the RANSAC pose, reproj 0
 *   matches < gate                no hypothesis is drawn at all (its consensus set cannot reach the gate): ok 0, n_inl 0, reproj 0
 * With the gate at 0 every candidate takes the first shape (tests/test_gpu_tick.py::test_inlier_gate_shapes_of_the_parity_tap). */
int reloc_tick_debug(reloc_ctx *ctx, int32_t *cand_ids, int32_t *n_cand, int32_t *n_matches,
                     int32_t *n_inl, int32_t *ok, double *reproj, double *Rt);
/* Parity tap (tests only): what the emit pass of the last solve on ctx left for candidate slot `slot` -- the slot's order
 * in reloc_tick_debug's cand_ids -- and so exactly what its PnP was given.  *n: the number of mutual matches; the first *n
 * entries of qidx (row within the record), tidx (current feature), dist (Hamming distance), in queryIdx order; obj (*n x 3,
 * the record's keypoints_3d_cam[qidx]) and img (*n x 2, the current keypoint xy[tidx]).  Every output pointer may be NULL;
 * arrays need room for the record's rows.  RELOC_E_ARG when slot is not in [0, n_cand) of that solve (read from the device
 * as reloc_tick_debug does).  Synchronises the context's stream; copies only, launches nothing.
 * The lists come in the orientation of the match policy in force at that solve (reloc_set_match_policy).  Under
 * RELOC_MATCH_RATIO: *n Lowe survivors, qidx = current feature, tidx = row within the record, obj = keypoints_3d_cam[tidx],
 * img = xy[qidx], arrays need room for max_feat entries; a record of fewer than min_matches rows keeps its list here and
 * is given no PnP (reloc_tick_debug reports n_matches 0 for it). */
int reloc_tick_debug_matches(reloc_ctx *ctx, int slot, int32_t *n, int32_t *qidx, int32_t *tidx, int32_t *dist,
                             float *obj, float *img);
/* Parity tap (tests only): the local candidate selection of a tick (M:293-302) alone, on the selected database -- the same
 * parameter block and the same launcher as a RELOC_TICK_LOCAL tick, no ORB, scan or PnP.  path: -1 = the kernels a tick of
 * this context would launch, 0 = the one-launch kernel (RELOC_E_ARG above 131072 records), 1 = the two stages.  ids_out: 32
 * entries, the first *n_out are the candidates in order.  Writes the context's candidate list, count and relocating flag, as
 * a tick's selection does, and nothing else; synchronises the context's stream. */
int reloc_debug_local_candidates(reloc_ctx *ctx, const double base_pose[7], int path, int32_t *ids_out, int32_t *n_out);
/* Parity tap (tests only): the whole-database count ranking (G:342-343) on counts the caller gives -- n_frames (1..8) arrays
 * of L int32, one launch through the launcher a tick uses (the single-frame kernel at n_frames 1, the batched one above).
 * Needs no database; its device scratch is allocated and freed inside the call.  Every count must be <= max_count (the size
 * of the ranking's histogram: in a tick the feature capacity or the rows of the largest record); 1 <= k <= 32, min_matches
 * >= 4, max_count <= 16254.  ids_out / counts_out: n_frames x 32, n_out: n_frames; all three are set to 0xA5A5A5A5 on the
 * device before the launch and copied back whole, so an entry the ranking did not write shows.  skip_in != NULL: the AUTO
 * arrangement -- frame f's n_out starts as skip_in[f] and is also the ranking's stand-down flag (non-zero: the local search
 * found candidates, the frame is not ranked and keeps every entry as it was).  Synchronises the context's stream. */
int reloc_debug_rank_counts(reloc_ctx *ctx, const int32_t *counts_host, int n_frames, int64_t L, int k, int64_t id_base,
                            int min_matches, int max_count, const int32_t *skip_in, int32_t *ids_out, int32_t *counts_out,
                            int32_t *n_out);
/* Parity tap (tests only): the device address of THIS context's per-record counts array of its selected database --
 * reloc_db_records entries of int32, the array the whole-database scans of this context's frames write (a single scan, its
 * frame of a batched launch) and their ranking reads.  Every holder of a database has its own: an adopter made by
 * reloc_db_share shares the records and counts into an array of its own.  NULL for a NULL context or while no database is
 * ready.  Launches nothing and copies nothing; valid until the database is uploaded, reserved, appended to, shared or
 * selected again. */
int32_t *reloc_db_counts_dev(reloc_ctx *ctx);
/* Sharded database (one rank per GPU): per-record mutual-match counts are local; the caller
 * exchanges the per-shard top-k (count, global id) lists and tells each rank which of ITS
 * records made the global top-k.  These two calls split reloc_tick_dev at that exchange. */
int reloc_tick_scan_dev(reloc_ctx *ctx, const uint8_t *img_dev, int w, int h, int order,
                        const double base_pose[7] /* NULL: no heading mask */,
                        int32_t *topk_ids_dev, int32_t *topk_counts_dev, int k);
int reloc_tick_solve_dev(reloc_ctx *ctx, const int32_t *cand_ids_dev, int n_cand,
                         const double base_pose[7], int check_consistency, uint64_t seed);
/* The same two halves for a BATCH of n <= 8 frames (BASELINE.json config 4) with the exchange kept in device memory: one
 * call per half, everything enqueued on the ONE stream the n contexts share (as for reloc_tick_batch_dev: one device, one
 * shard through reloc_db_share, equal capacity and parameters), so the caller's collective (RCCL all-gather of the rows
 * below) can be enqueued on that same stream between them and the host never waits inside a batch.
 *   scan half:  ORB per frame, ONE scan launch for the n frames, per-frame ranking.  scan_out_dev: n rows of 2k + 2
 *               int32 = k GLOBAL record ids (id_base + local id, -1 padded), k mutual-match counts, the frame's feature
 *               count, one pad word the call never writes.  base_poses: n x 7 (heading mask, G:329-330) or NULL.
 *   merge:      what every rank computes from the gathered rows (all_scan_dev: `world` blocks `stride_rank` int32 apart,
 *               each n rows as above): per frame the k best (count desc, global id desc; G:342-343) -> win_gid (n x k,
 *               -1 padded), cand_local (n x k: local ids of the winners THIS rank owns, -1 elsewhere), n_feat (n: the
 *               largest feature count any rank reported, -1 from ranks without records).
 *   solve half: match lists + PnP + gates (relocation gates, no consistency check, G:381-382,424) for the owned winners of
 *               every frame; the 96-byte result record of frame f is stored at res_out + 96 f by the tick's last kernel
 *               (device or pinned host memory). */
int reloc_shard_scan_batch_dev(reloc_ctx *const *ctxs, int n, const uint8_t *const *imgs_dev, int w, int h, int order,
                               const double *base_poses, int k, int64_t id_base, int32_t *scan_out_dev);
int reloc_shard_merge_dev(reloc_ctx *ctx, const int32_t *all_scan_dev, int world, int64_t stride_rank, int n, int k,
                          int64_t id_base, int64_t n_local, int32_t *win_gid_dev, int32_t *cand_local_dev,
                          int32_t *n_feat_dev);
int reloc_shard_solve_batch_dev(reloc_ctx *const *ctxs, int n, const int32_t *cand_local_dev, int k,
                                const double *base_poses, const uint64_t *seeds, void *res_out);

#ifdef __cplusplus
}
#endif
#endif /* RELOC_H */
