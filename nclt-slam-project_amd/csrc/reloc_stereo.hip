// reloc_stereo.hip -- stereo depth on gfx950: the depth of the ORB keypoints from the other eye of a rectified pair (sparse;
// include/reloc_spec.h, "STEREO"), the stereo settings of a context, and what every stereo pass does with its pair of contexts
// (stereo_pair_check, stereo_gray_planes).  The depth of every pixel (dense, with its optional semi-global aggregation) is
// reloc_stereo_dense.hip; the decision both make per pixel is reloc_stereo_match.h.  The matcher is this project's own; the
// spec states it in integers and tests/stereo_ref.py restates it bit for bit.
//   k_stereo_depth   one wave per keypoint, lanes over disparities, 64 per pass (num_disparities > 64: further passes of the
//                    same wave).  Per pass the 11 rows of the searched eye that the 64 candidates cover (74 bytes each) and
//                    the 11 x 11 patch of the other eye are staged in LDS, about 1 KB per wave.  A lane's patch row is three
//                    dwords cut out of four aligned LDS dwords (v_alignbyte), the absolute differences are four per
//                    instruction (v_sad_u8).  Four neighbouring lanes read the same dwords, 64 lanes span 17: no bank conflict.
//                    (cost, disparity) travel as one integer key, cost << 11 | d, and are reduced with min in the DPP network,
//                    so the lowest disparity wins a tie by the reduction itself.  The costs of a wave stay in registers (one
//                    per pass); the parabola's neighbours are read back from the lanes that hold them.
//                    Every branch on a status is wave-uniform; a workgroup is one wave, so its barriers cost nothing.
//                    k_stereo_depth<COST>: with the census ("STEREO, census") the planes are the census planes of
//                    reloc_census.hip, staged the same way, and a dword's cost is an xor and a popcount (stereo_cost4).
// Each eye has its own row stride (a pyramid level or a stage's plane: (w + 63) & ~63; a dense gray plane or a caller's mono8
// frame: w; reloc_stereo_depth: the caller's).  The bytes are staged one by one through the cache: rows start at any
// alignment, and a byte outside 0 <= x < w, row padding included, is never fetched.
#include "reloc_stereo_match.h"
#include "reloc_pixels.h"

constexpr int STRIP_DW = 20;          // dwords per staged row: 63 + SP bytes, read as 4 dwords from dword (63 >> 2)
constexpr int PATCH_DW = 3;           // dwords per patch row, the twelfth byte zero

// rows v - R .. v + R of img, bytes x0 .. x0 + 4 ndw - 1, as dwords dst[row * ndw + k]; a byte outside 0 <= x < w is 0 and is
// not fetched; patch: the bytes behind the eleventh are 0 as well
__device__ __forceinline__ void stereo_stage(const uint8_t *__restrict__ img, int stride, int w, int v, int x0, int ndw, bool patch,
                                             uint32_t *dst, int lane)
{
    for (int t = lane; t < SP * ndw; t += 64) {
        const int j = t / ndw, k = t - j * ndw;
        const uint8_t *row = img + (size_t)(v - SR + j) * stride;
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int x = x0 + 4 * k + b;
            if (x >= 0 && x < w && !(patch && 4 * k + b >= SP)) word |= (uint32_t)row[x] << (8 * b);
        }
        dst[t] = word;
    }
}

// the cost of four bytes against four bytes on top of acc: the SAD of gray bytes, or the Hamming distance of census bytes
template <int COST>
__device__ __forceinline__ unsigned stereo_cost4(unsigned a, unsigned b, unsigned acc)
{
    if constexpr (COST == RELOC_STEREO_COST_CENSUS) return acc + (unsigned)__builtin_popcount(a ^ b);      // v_xor, v_bcnt with its addend
    else return __builtin_amdgcn_sad_u8(a, b, acc);
}

// cost of the staged patch and the SP x SP window whose first byte is byte `off` of the staged rows
template <int COST>
__device__ __forceinline__ int stereo_cost(const uint32_t *strip, const uint32_t *patch, int off)
{
    const int q = off >> 2;
    const unsigned sh = (unsigned)off & 3u;
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < SP; ++j) {
        const uint32_t *s = strip + j * STRIP_DW + q;
        const uint32_t w0 = s[0], w1 = s[1], w2 = s[2], w3 = s[3];
        c = stereo_cost4<COST>(__builtin_amdgcn_alignbyte(w1, w0, sh), patch[PATCH_DW * j], c);
        c = stereo_cost4<COST>(__builtin_amdgcn_alignbyte(w2, w1, sh), patch[PATCH_DW * j + 1], c);
        c = stereo_cost4<COST>(__builtin_amdgcn_alignbyte(w3, w2, sh) & 0x00FFFFFFu, patch[PATCH_DW * j + 2], c);
    }
    return (int)c;
}

// keypoint blockIdx.x of xy; count: their number on the device (the frame's own keypoints, at most n_max) or NULL: n_max.
// COST: the planes are gray planes (SAD) or census planes
template <int COST>
__global__ __launch_bounds__(64) void k_stereo_depth(const uint8_t *__restrict__ left, int lstride, const uint8_t *__restrict__ right,
                                                     int rstride, const float *__restrict__ xy, const int32_t *__restrict__ count,
                                                     int n_max, StereoParams p, uint16_t *__restrict__ o_mm,
                                                     float *__restrict__ o_disp, uint8_t *__restrict__ o_status)
{
    RELOC_SMALL_KERNEL_PRIO();
    __shared__ uint32_t s_strip[SP * STRIP_DW];
    __shared__ uint32_t s_patch[SP * PATCH_DW];
    const int lane = threadIdx.x, i = blockIdx.x;
    const int n = count ? min(*count, n_max) : n_max;
    if (i >= n) return;
    const int u = (int)rintf(xy[2 * i]), v = (int)rintf(xy[2 * i + 1]);
    const int dmin = p.min_disp;
    const int dhi = min(dmin + p.num_disp - 1, u - SR);          // largest member of D
    StereoPick s = {RELOC_STEREO_BORDER, 0, 0, 0, 0};
    if (u >= SR && u < p.w - SR && v >= SR && v < p.h - SR) {
        // ---- step 3: the costs of D, lane l of pass q holds d = dmin + 64 q + l; a keypoint that fails step 2 stages nothing ----
        int cost[STEREO_PASSES] = {};
        if (stereo_range_ok(dmin, dhi)) {
            const int npass = (dhi - dmin + 64) >> 6;
            stereo_stage(left, lstride, p.w, v, u - SR, PATCH_DW, true, s_patch, lane);
#pragma unroll
            for (int q = 0; q < STEREO_PASSES; ++q) {
                if (q < npass) {
                    if (q) __syncthreads();                       // the previous pass has read the strip
                    stereo_stage(right, rstride, p.w, v, u - dmin - 64 * q - 63 - SR, STRIP_DW, false, s_strip, lane);
                    __syncthreads();
                    cost[q] = stereo_cost<COST>(s_strip, s_patch, 63 - lane);
                }
            }
        }
        s = stereo_select<STEREO_PASSES>(cost, dmin, dhi, p.uniq, lane);
    }
    int status = s.status;
    if (status == RELOC_STEREO_OK && p.lr) {
        // ---- step 6: the same search from the right eye's patch at xr over the left eye ----
        const int xr = u - s.dstar;
        const int dhi2 = min(dmin + p.num_disp - 1, p.w - SR - 1 - xr);      // >= dstar: D' is never empty
        const int npass = (dhi2 - dmin + 64) >> 6;
        unsigned key = KEY_NONE;
        __syncthreads();
        stereo_stage(right, rstride, p.w, v, xr - SR, PATCH_DW, true, s_patch, lane);
        for (int q = 0; q < npass; ++q) {
            const int d0 = dmin + 64 * q, d = d0 + lane;
            if (q) __syncthreads();
            stereo_stage(left, lstride, p.w, v, xr + d0 - SR, STRIP_DW, false, s_strip, lane);
            __syncthreads();
            const int cq = stereo_cost<COST>(s_strip, s_patch, lane);
            if (d <= dhi2) key = min(key, stereo_key(cq, d));
        }
        key = wave_min_u32(key);
        if (abs((int)(key & 0x7FFu) - s.dstar) > 1) status = RELOC_STEREO_LR;
    }
    StereoDepth z = {status, 0, 0.f};
    if (status == RELOC_STEREO_OK) z = stereo_depth_of(s.dstar, s.a, s.b, s.c, p.fx, p.baseline);
    if (lane == 0) {
        o_mm[i] = z.mm;
        o_disp[i] = z.disp;
        o_status[i] = (uint8_t)z.status;
    }
}

// cost: RELOC_STEREO_COST_*; with the census both planes go through k_census first, inside the same stopwatch bracket
static int stereo_launch(reloc_ctx *ctx, const uint8_t *left, int lstride, const uint8_t *right, int rstride, const float *xy,
                         const int32_t *count, int n_max, const StereoParams &p, int cost, uint16_t *mm, float *disp, uint8_t *status)
{
    if (cost)
        if (int rc = stereo_census_alloc(ctx)) return rc;
    reloc_prof_begin(ctx, RELOC_PROF_STEREO);
    if (cost) stereo_census_launch(ctx, left, lstride, right, rstride, p.w, p.h);
    hipLaunchKernelGGL(cost ? k_stereo_depth<RELOC_STEREO_COST_CENSUS> : k_stereo_depth<RELOC_STEREO_COST_SAD>, dim3(n_max), dim3(64), 0,
                       ctx->stream, left, lstride, right, rstride, xy, count, n_max, p, mm, disp, status);
    reloc_prof_end(ctx, RELOC_PROF_STEREO);
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

static int stereo_cost_check(int cost)
{
    if (cost != RELOC_STEREO_COST_SAD && cost != RELOC_STEREO_COST_CENSUS) {
        reloc_set_error("bad argument: stereo cost %d outside 0..1", cost);
        return RELOC_E_ARG;
    }
    return RELOC_OK;
}

static int stereo_args_check(double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check, bool may_be_off)
{
    if (!(baseline_m - baseline_m == 0.0) || baseline_m < 0.0 || (!may_be_off && baseline_m == 0.0)) {
        reloc_set_error("bad argument: stereo baseline_m %g is not finite and %s 0", baseline_m, may_be_off ? ">=" : ">");
        return RELOC_E_ARG;
    }
    if (min_disparity < 0 || min_disparity > RELOC_STEREO_MIN_DISPARITY_MAX) {
        reloc_set_error("bad argument: stereo min_disparity %d outside 0..%d", min_disparity, RELOC_STEREO_MIN_DISPARITY_MAX);
        return RELOC_E_ARG;
    }
    if (num_disparities < RELOC_STEREO_NUM_DISP_MIN || num_disparities > RELOC_STEREO_NUM_DISP_MAX) {
        reloc_set_error("bad argument: stereo num_disparities %d outside %d..%d", num_disparities, RELOC_STEREO_NUM_DISP_MIN, RELOC_STEREO_NUM_DISP_MAX);
        return RELOC_E_ARG;
    }
    if (uniqueness < 0 || uniqueness > RELOC_STEREO_UNIQUENESS_MAX) {
        reloc_set_error("bad argument: stereo uniqueness %d outside 0..%d", uniqueness, RELOC_STEREO_UNIQUENESS_MAX);
        return RELOC_E_ARG;
    }
    if (lr_check != 0 && lr_check != 1) { reloc_set_error("bad argument: stereo lr_check %d outside 0..1", lr_check); return RELOC_E_ARG; }
    return RELOC_OK;
}

static int stereo_sgm_args_check(const StereoSgm &g)
{
    if (g.mask < 1 || g.mask > 255) { reloc_set_error("bad argument: stereo sgm path_mask %d outside 1..255", g.mask); return RELOC_E_ARG; }
    if (g.p1 < 0 || g.p2 < g.p1 || g.p2 > RELOC_STEREO_SGM_P2_MAX) {
        reloc_set_error("bad argument: stereo sgm penalties p1 %d, p2 %d outside 0 <= p1 <= p2 <= %d", g.p1, g.p2, RELOC_STEREO_SGM_P2_MAX);
        return RELOC_E_ARG;
    }
    return RELOC_OK;
}

int stereo_call_check(const reloc_ctx *ctx, int w, int h, double fx, double baseline_m, int min_disparity, int num_disparities,
                      int uniqueness, int lr_check, int cost, const StereoSgm *sgm)
{
    if (!(fx - fx == 0.0) || fx <= 0.0) { reloc_set_error("bad argument: stereo fx %g is not finite and > 0", fx); return RELOC_E_ARG; }
    if (int rc = stereo_args_check(baseline_m, min_disparity, num_disparities, uniqueness, lr_check, false)) return rc;
    if (int rc = stereo_cost_check(cost)) return rc;
    if (sgm)
        if (int rc = stereo_sgm_args_check(*sgm)) return rc;
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    return RELOC_OK;
}

RELOC_API int reloc_set_stereo(reloc_ctx *ctx, double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check)
{
    ARG_CHECK_CTX(ctx, true, "reloc_set_stereo");
    StereoState &s = ctx->stereo;
    if (baseline_m == 0.0) {       // off: the setting of a new context
        s.baseline = 0.0; s.min_disp = 0; s.num_disp = RELOC_STEREO_NUM_DISP_DEFAULT; s.uniq = RELOC_STEREO_UNIQUENESS_DEFAULT; s.lr = 1;
        return RELOC_OK;
    }
    if (int rc = stereo_args_check(baseline_m, min_disparity, num_disparities, uniqueness, lr_check, true)) return rc;
    if (s.baseline == baseline_m && s.min_disp == min_disparity && s.num_disp == num_disparities && s.uniq == uniqueness && s.lr == lr_check)
        return RELOC_OK;       // nothing changes
    if (!s.left_ready) {
        // first enable: the block, zeroed in front of the plane, and both events; a failure leaves stereo off
        if (int rc = s.block.layout(ctx, [&](BlockCarver &c) { stereo_sparse_lines(c, s, ctx->max_feat, (int64_t)ctx->max_w * ctx->max_h); })) return rc;
        HIP_TRY(hipMemsetAsync(s.block.p, 0, (size_t)(s.plane - s.block.p), ctx->stream));
        if ((!s.right_done && hipEventCreateWithFlags(&s.right_done, hipEventDisableTiming) != hipSuccess) ||
            (!s.left_ready && hipEventCreateWithFlags(&s.left_ready, hipEventDisableTiming) != hipSuccess)) {
            stereo_release(ctx);
            reloc_set_error("stereo: event creation failed");
            return RELOC_E_HIP;
        }
    }
    s.baseline = baseline_m; s.min_disp = min_disparity; s.num_disp = num_disparities; s.uniq = uniqueness; s.lr = lr_check;
    return RELOC_OK;
}

RELOC_API int reloc_get_stereo(reloc_ctx *ctx, double *baseline_m, int32_t *min_disparity, int32_t *num_disparities, int32_t *uniqueness,
                               int32_t *lr_check)
{
    ARG_CHECK(ctx, "reloc_get_stereo");
    const StereoState &s = ctx->stereo;
    if (baseline_m) *baseline_m = s.baseline;
    if (min_disparity) *min_disparity = s.min_disp;
    if (num_disparities) *num_disparities = s.num_disp;
    if (uniqueness) *uniqueness = s.uniq;
    if (lr_check) *lr_check = s.lr;
    return RELOC_OK;
}

RELOC_API int reloc_set_stereo_sgm(reloc_ctx *ctx, int paths, int p1, int p2)
{
    ARG_CHECK_CTX(ctx, true, "reloc_set_stereo_sgm");
    StereoState &s = ctx->stereo;
    if (paths == 0) {          // off: the setting of a new context
        s.sgm_paths = 0; s.sgm_p1 = RELOC_STEREO_SGM_P1_DEFAULT; s.sgm_p2 = RELOC_STEREO_SGM_P2_DEFAULT;
        return RELOC_OK;
    }
    if (paths != 4 && paths != 8) { reloc_set_error("bad argument: stereo sgm paths %d is not 0, 4 or 8", paths); return RELOC_E_ARG; }
    if (int rc = stereo_sgm_args_check(StereoSgm{0xFF, p1, p2})) return rc;
    s.sgm_paths = paths; s.sgm_p1 = p1; s.sgm_p2 = p2;
    return RELOC_OK;
}

RELOC_API int reloc_get_stereo_sgm(reloc_ctx *ctx, int32_t *paths, int32_t *p1, int32_t *p2)
{
    ARG_CHECK(ctx, "reloc_get_stereo_sgm");
    const StereoState &s = ctx->stereo;
    if (paths) *paths = s.sgm_paths;
    if (p1) *p1 = s.sgm_p1;
    if (p2) *p2 = s.sgm_p2;
    return RELOC_OK;
}

RELOC_API int reloc_set_stereo_cost(reloc_ctx *ctx, int cost)
{
    ARG_CHECK_CTX(ctx, true, "reloc_set_stereo_cost");
    if (int rc = stereo_cost_check(cost)) return rc;
    ctx->stereo.cost = cost;
    return RELOC_OK;
}

RELOC_API int reloc_get_stereo_cost(reloc_ctx *ctx, int32_t *cost)
{
    ARG_CHECK(ctx, "reloc_get_stereo_cost");
    if (cost) *cost = ctx->stereo.cost;
    return RELOC_OK;
}

void stereo_release(reloc_ctx *ctx)
{
    StereoState &s = ctx->stereo;
    if (s.right_done) (void)hipEventDestroy(s.right_done);
    if (s.left_ready) (void)hipEventDestroy(s.left_ready);
    s.right_done = s.left_ready = nullptr;
    s.ran = false;
}

// the stateless per-keypoint call: two gray planes of the caller's with one stride, explicit parameters
static int stereo_sparse_call(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, const float *xy, int n,
                              double fx, double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check, int cost,
                              uint16_t *depth_mm, float *disparity, uint8_t *status)
{
    if (int rc = stereo_call_check(ctx, w, h, fx, baseline_m, min_disparity, num_disparities, uniqueness, lr_check, cost, nullptr)) return rc;
    if (n == 0) return RELOC_OK;
    // the planes go to the device as they lie at the caller's, padding included, and the kernel walks the caller's stride
    const int64_t bytes = (int64_t)(h - 1) * stride + w;
    HostStaging st{ctx};
    uint8_t *dl = st.slot<uint8_t>(0, bytes), *dr = st.slot<uint8_t>(1, bytes);
    float *dxy = st.upload_slot(2, xy, (int64_t)n * 2);
    uint8_t *out = st.slot<uint8_t>(3, (int64_t)n * 7);
    if (st.rc) return st.finish();
    float *o_disp = (float *)out;
    uint16_t *o_mm = (uint16_t *)(out + (int64_t)n * 4);
    uint8_t *o_st = out + (int64_t)n * 6;
    st.upload(dl, left, bytes);
    st.upload(dr, right, bytes);
    const StereoParams p = {fx, baseline_m, w, h, min_disparity, num_disparities, uniqueness, lr_check};
    st.run([&] { return stereo_launch(ctx, dl, stride, dr, stride, dxy, nullptr, n, p, cost, o_mm, o_disp, o_st); });
    st.download(disparity, o_disp, (int64_t)n * 4);
    st.download(depth_mm, o_mm, (int64_t)n * 2);
    st.download(status, o_st, n);
    return st.finish();
}

RELOC_API int reloc_stereo_depth(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, const float *xy,
                                 int n, double fx, double baseline_m, int min_disparity, int num_disparities, int uniqueness,
                                 int lr_check, uint16_t *depth_mm, float *disparity, uint8_t *status)
{
    ARG_CHECK_CTX(ctx, left && right && w >= SP && h >= SP && stride >= w && n >= 0 && (n == 0 || (xy && depth_mm && disparity && status)),
                  "reloc_stereo_depth");
    return stereo_sparse_call(ctx, left, right, w, h, stride, xy, n, fx, baseline_m, min_disparity, num_disparities, uniqueness, lr_check,
                              RELOC_STEREO_COST_SAD, depth_mm, disparity, status);
}

RELOC_API int reloc_stereo_depth_cost(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, const float *xy,
                                      int n, double fx, double baseline_m, int min_disparity, int num_disparities, int uniqueness,
                                      int lr_check, int cost, uint16_t *depth_mm, float *disparity, uint8_t *status)
{
    ARG_CHECK_CTX(ctx, left && right && w >= SP && h >= SP && stride >= w && n >= 0 && (n == 0 || (xy && depth_mm && disparity && status)),
                  "reloc_stereo_depth_cost");
    return stereo_sparse_call(ctx, left, right, w, h, stride, xy, n, fx, baseline_m, min_disparity, num_disparities, uniqueness, lr_check,
                              cost, depth_mm, disparity, status);
}

int stereo_pair_check(reloc_ctx *ctx, reloc_ctx *right, int w, int h, int *ww, int *wh)
{
    if (int rc = stereo_pair_entry(ctx, right, w, h)) return rc;
    if (right->device != ctx->device || right->prm.gray_coeff_bits != ctx->prm.gray_coeff_bits) {
        reloc_set_error("stereo: the right eye's context is on another device or has another gray_coeff_bits");
        return RELOC_E_STATE;
    }
    reloc_ctx *pair[2] = {ctx, right};
    *ww = w; *wh = h;
    if (int rc = image_chain_check(pair, 2, true, ww, wh)) return rc;
    return image_chain_check_prepared(pair, 1, 2, true, *ww, *wh);
}

int stereo_gray_planes(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *lsrc, const uint8_t *rsrc, int w, int h, int ww, int wh,
                       int order, const uint8_t *plane[2], int stride[2])
{
    StereoState &s = ctx->stereo;
    // eye e: c's frame (w x h as handed in) through the gray half of its chain; into dst when no stage ran on a 3-channel frame
    auto eye = [&](int e, reloc_ctx *c, const uint8_t *src, uint8_t *dst) {
        const uint8_t *planes[RELOC_BATCH_MAX];
        const uint8_t *const *srcs = &src;
        int channels = 1;
        stride[e] = w * image_chain_frame_bpp(c);
        if (int rc = image_chain_gray(&c, 1, true, &srcs, w, h, ww, wh, &stride[e], &channels, gray_flags(c, order), planes)) return rc;
        plane[e] = srcs[0];
        if (channels == 3) {
            if (int rc = image_gray_plain(c, plane[e], ww, wh, stride[e], order, dst)) return rc;
            plane[e] = dst; stride[e] = ww;
        }
        return (int)RELOC_OK;
    };
    HIP_TRY(hipEventRecord(s.left_ready, ctx->stream));
    HIP_TRY(hipStreamWaitEvent(right->stream, s.left_ready, 0));
    if (lsrc)
        if (int rc = eye(0, ctx, lsrc, s.dense.left)) return rc;
    if (int rc = eye(1, right, rsrc, s.plane)) return rc;
    HIP_TRY(hipEventRecord(s.right_done, right->stream));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, s.right_done, 0));
    return RELOC_OK;
}

int stereo_frame(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *img_right_dev, int w, int h, int order, int *ww, int *wh)
{
    StereoState &s = ctx->stereo;
    if (int rc = stereo_pair_check(ctx, right, w, h, ww, wh)) return rc;
    if (ctx->orb.w != *ww || ctx->orb.h != *wh) {
        reloc_set_error("stereo: the left eye's last ORB frame is %dx%d, the right eye's working frame %dx%d", ctx->orb.w, ctx->orb.h, *ww, *wh);
        return RELOC_E_STATE;
    }
    const uint8_t *plane[2];
    int stride[2];
    if (int rc = stereo_gray_planes(ctx, right, nullptr, img_right_dev, w, h, *ww, *wh, order, plane, stride)) return rc;
    const OrbLevel &L0 = ctx->orb.tab.lev[0];       // level 0 of the pyramid is the chain's output (the blurred levels live in buf.blur)
    const StereoParams p = {ctx->cam.K4[0], s.baseline, *ww, *wh, s.min_disp, s.num_disp, s.uniq, s.lr};
    if (int rc = stereo_launch(ctx, ctx->orb.buf.pyr + L0.off, L0.stride, plane[1], stride[1], ctx->orb.buf.f_xy, ctx->orb.buf.f_count,
                               ctx->max_feat, p, s.cost, s.mm, s.disp, s.status)) return rc;
    s.ran = true;
    return RELOC_OK;
}

RELOC_API int reloc_stereo_debug(reloc_ctx *ctx, uint16_t *depth_mm, float *disparity, uint8_t *status, int32_t *n)
{
    ARG_CHECK_CTX(ctx, n, "reloc_stereo_debug");
    const StereoState &s = ctx->stereo;
    if (!s.disp || !s.ran) { reloc_set_error("no stereo pass on this context yet"); return RELOC_E_STATE; }
    HostStaging st{ctx};
    int32_t k = st.count(ctx->orb.buf.f_count);
    k = k < ctx->max_feat ? k : ctx->max_feat;
    if (k > 0) {
        if (depth_mm) st.download(depth_mm, s.mm, (int64_t)k * 2);
        if (disparity) st.download(disparity, s.disp, (int64_t)k * 4);
        if (status) st.download(status, s.status, k);
    }
    if (int rc = st.finish()) return rc;
    *n = k;
    return RELOC_OK;
}
