// reloc_stereo.hip -- stereo depth on gfx950: the depth of the ORB keypoints (sparse) or of every pixel (dense, second half of
// this file, with its optional semi-global aggregation) from the other eye of a rectified pair (include/reloc_spec.h, "STEREO",
// "STEREO, dense", "STEREO, semi-global").  The matcher is this project's own; the spec states it in integers and
// tests/stereo_ref.py restates it bit for bit.
//   k_stereo_depth   one wave per keypoint, lanes over disparities, 64 per pass (num_disparities > 64: further passes of the
//                    same wave).  Per pass the 11 rows of the searched eye that the 64 candidates cover (74 bytes each) and
//                    the 11 x 11 patch of the other eye are staged in LDS, about 1 KB per wave.  A lane's patch row is three
//                    dwords cut out of four aligned LDS dwords (v_alignbyte), the absolute differences are four per
//                    instruction (v_sad_u8).  Four neighbouring lanes read the same dwords, 64 lanes span 17: no bank conflict.
//                    (cost, disparity) travel as one integer key, cost << 11 | d, and are reduced with min in the DPP network,
//                    so the lowest disparity wins a tie by the reduction itself.  The costs of a wave stay in registers (one
//                    per pass); the parabola's neighbours are read back from the lanes that hold them.
//                    Every branch on a status is wave-uniform; a workgroup is one wave, so its barriers cost nothing.
// Each eye has its own row stride (a pyramid level or a stage's plane: (w + 63) & ~63; a dense gray plane or a caller's mono8
// frame: w; reloc_stereo_depth: the caller's).  The bytes are staged one by one through the cache: rows start at any
// alignment, and a byte outside 0 <= x < w, row padding included, is never fetched.
#include "reloc_teach.h"
#include "reloc_pixels.h"

constexpr int SR = RELOC_STEREO_R, SP = 2 * RELOC_STEREO_R + 1;     // radius and side of the patch
constexpr int STRIP_DW = 20;          // dwords per staged row: 63 + SP bytes, read as 4 dwords from dword (63 >> 2)
constexpr int PATCH_DW = 3;           // dwords per patch row, the twelfth byte zero
constexpr int STEREO_PASSES = RELOC_STEREO_NUM_DISP_MAX / 64;
constexpr unsigned KEY_NONE = 0xFFFFFFFFu;
constexpr uint16_t SGM_NONE = 0xFFFFu;   // an entry of the semi-global cost volume outside D(u): above every SAD cost (30 855)
static_assert(SP == 11 && SP * SP * 255 < (1 << 15) && RELOC_STEREO_MIN_DISPARITY_MAX + RELOC_STEREO_NUM_DISP_MAX < (1 << 11),
              "cost << 11 | disparity is a 26-bit key");

struct StereoParams {
    double fx, baseline;
    int w, h;
    int min_disp, num_disp, uniq, lr;
};

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

// SAD of the staged patch and the SP x SP window whose first byte is byte `off` of the staged rows
__device__ __forceinline__ int stereo_cost(const uint32_t *strip, const uint32_t *patch, int off)
{
    const int q = off >> 2;
    const unsigned sh = (unsigned)off & 3u;
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < SP; ++j) {
        const uint32_t *s = strip + j * STRIP_DW + q;
        const uint32_t w0 = s[0], w1 = s[1], w2 = s[2], w3 = s[3];
        c = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w1, w0, sh), patch[PATCH_DW * j], c);
        c = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w2, w1, sh), patch[PATCH_DW * j + 1], c);
        c = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w3, w2, sh) & 0x00FFFFFFu, patch[PATCH_DW * j + 2], c);
    }
    return (int)c;
}

// pass-th register of a lane's costs (pass is wave-uniform)
__device__ __forceinline__ int stereo_pick(const int (&cost)[STEREO_PASSES], int pass)
{
    int r = cost[0];
#pragma unroll
    for (int p = 1; p < STEREO_PASSES; ++p) r = pass == p ? cost[p] : r;
    return r;
}

// keypoint blockIdx.x of xy; count: their number on the device (the frame's own keypoints, at most n_max) or NULL: n_max
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
    int status = RELOC_STEREO_OK;
    uint16_t mm_out = 0;
    float disp_out = 0.f;
    const int u = (int)rintf(xy[2 * i]), v = (int)rintf(xy[2 * i + 1]);
    const int dmin = p.min_disp;
    const int dhi = min(dmin + p.num_disp - 1, u - SR);          // largest member of D
    int dstar = 0, a = 0, b = 0, c = 0;
    if (!(u >= SR && u < p.w - SR && v >= SR && v < p.h - SR)) status = RELOC_STEREO_BORDER;
    else if (dhi - dmin + 1 < 3) status = RELOC_STEREO_RANGE;
    else {
        // ---- steps 3-5: the costs of D, lane l of pass q holds d = dmin + 64 q + l ----
        const int npass = (dhi - dmin + 64) >> 6;
        int cost[STEREO_PASSES];
        unsigned key = KEY_NONE;
        stereo_stage(left, lstride, p.w, v, u - SR, PATCH_DW, true, s_patch, lane);
#pragma unroll
        for (int q = 0; q < STEREO_PASSES; ++q) {
            cost[q] = 0;
            if (q < npass) {
                const int d0 = dmin + 64 * q, d = d0 + lane;
                if (q) __syncthreads();                           // the previous pass has read the strip
                stereo_stage(right, rstride, p.w, v, u - d0 - 63 - SR, STRIP_DW, false, s_strip, lane);
                __syncthreads();
                cost[q] = stereo_cost(s_strip, s_patch, 63 - lane);
                if (d <= dhi) key = min(key, ((unsigned)cost[q] << 11) | (unsigned)d);
            }
        }
        key = wave_min_u32(key);
        dstar = (int)(key & 0x7FFu);
        b = (int)(key >> 11);
        if (dstar == dmin || dstar == dhi) status = RELOC_STEREO_EDGE;
        else {
            unsigned key2 = KEY_NONE;
#pragma unroll
            for (int q = 0; q < STEREO_PASSES; ++q) {
                const int d = dmin + 64 * q + lane;
                if (q < npass && d <= dhi && abs(d - dstar) >= 2) key2 = min(key2, ((unsigned)cost[q] << 11) | (unsigned)d);
            }
            key2 = wave_min_u32(key2);
            if (key2 != KEY_NONE && (int)(key2 >> 11) * (100 - p.uniq) <= b * 100) status = RELOC_STEREO_UNIQUENESS;
            else {
                const int ia = dstar - 1 - dmin, ic = dstar + 1 - dmin;
                a = __builtin_amdgcn_readlane(stereo_pick(cost, ia >> 6), ia & 63);
                c = __builtin_amdgcn_readlane(stereo_pick(cost, ic >> 6), ic & 63);
            }
        }
    }
    if (status == RELOC_STEREO_OK && p.lr) {
        // ---- step 6: the same search from the right eye's patch at xr over the left eye ----
        const int xr = u - dstar;
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
            const int cq = stereo_cost(s_strip, s_patch, lane);
            if (d <= dhi2) key = min(key, ((unsigned)cq << 11) | (unsigned)d);
        }
        key = wave_min_u32(key);
        if (abs((int)(key & 0x7FFu) - dstar) > 1) status = RELOC_STEREO_LR;
    }
    if (status == RELOC_STEREO_OK) {
        // ---- steps 7, 8 ----
        const int den = a + c - 2 * b;
        const float delta = den <= 0 ? 0.f : __fdiv_rn((float)(a - c), (float)(2 * den));
        const float disp = __fadd_rn((float)dstar, delta);
        const double z = __ddiv_rn(__dmul_rn(p.fx, p.baseline), (double)disp);
        const double mm = rint(__dmul_rn(z, 1000.0));
        if (mm > 65535.0) status = RELOC_STEREO_FAR;
        else { mm_out = (uint16_t)mm; disp_out = disp; }
    }
    if (lane == 0) {
        o_mm[i] = mm_out;
        o_disp[i] = disp_out;
        o_status[i] = (uint8_t)status;
    }
}

static int stereo_launch(reloc_ctx *ctx, const uint8_t *left, int lstride, const uint8_t *right, int rstride, const float *xy,
                         const int32_t *count, int n_max, const StereoParams &p, uint16_t *mm, float *disp, uint8_t *status)
{
    reloc_prof_begin(ctx, RELOC_PROF_STEREO);
    hipLaunchKernelGGL(k_stereo_depth, dim3(n_max), dim3(64), 0, ctx->stream, left, lstride, right, rstride, xy, count, n_max, p, mm, disp, status);
    reloc_prof_end(ctx, RELOC_PROF_STEREO);
    HIP_TRY(hipGetLastError());
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

void stereo_release(reloc_ctx *ctx)
{
    StereoState &s = ctx->stereo;
    if (s.right_done) (void)hipEventDestroy(s.right_done);
    if (s.left_ready) (void)hipEventDestroy(s.left_ready);
    s.right_done = s.left_ready = nullptr;
    s.ran = false;
}

RELOC_API int reloc_stereo_depth(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, const float *xy,
                                 int n, double fx, double baseline_m, int min_disparity, int num_disparities, int uniqueness,
                                 int lr_check, uint16_t *depth_mm, float *disparity, uint8_t *status)
{
    ARG_CHECK_CTX(ctx, left && right && w >= SP && h >= SP && stride >= w && n >= 0 && (n == 0 || (xy && depth_mm && disparity && status)),
                  "reloc_stereo_depth");
    if (!(fx - fx == 0.0) || fx <= 0.0) { reloc_set_error("bad argument: stereo fx %g is not finite and > 0", fx); return RELOC_E_ARG; }
    if (int rc = stereo_args_check(baseline_m, min_disparity, num_disparities, uniqueness, lr_check, false)) return rc;
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
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
    st.run([&] { return stereo_launch(ctx, dl, stride, dr, stride, dxy, nullptr, n, p, o_mm, o_disp, o_st); });
    st.download(disparity, o_disp, (int64_t)n * 4);
    st.download(depth_mm, o_mm, (int64_t)n * 2);
    st.download(status, o_st, n);
    return st.finish();
}

// What a stereo pass checks of its pair of contexts before it enqueues anything: what an entry point checks (stereo_pair_entry),
// then two contexts of one device and one gray conversion, the two chains in agreement as in a batch; *ww x *wh: the working frame.
static int stereo_pair_check(reloc_ctx *ctx, reloc_ctx *right, int w, int h, int *ww, int *wh)
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

// The gray planes of a pass, plane[e] with rows of stride[e] bytes, e = 1 the right eye: the right eye's chain on right's stream,
// the left eye's (lsrc == NULL: none, plane[0] is not written) on ctx's.  The streams are ordered by events in both directions:
// right's goes on behind what ctx's holds so far -- the copy that brought the right frame (a _dev caller orders its frames on
// ctx's stream) and the last stereo kernel, which still reads the right chain's planes -- and ctx's behind the right eye's chain.
static int stereo_gray_planes(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *lsrc, const uint8_t *rsrc, int w, int h, int ww, int wh,
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
                               ctx->max_feat, p, s.mm, s.disp, s.status)) return rc;
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

// ---------------------------------------------------------------------------------------------------
// Dense stereo depth (include/reloc_spec.h, "STEREO, dense"): the same specification at every integer pixel.
//   k_stereo_dense<NP>     a workgroup of four waves takes DT_W output columns of one row, a wave 64 of them; lanes over
//                          disparities, NP = ceil(num_disparities / 64) of them per lane.  The 11 rows that the row's windows
//                          cover are staged in LDS column by column: the 11 bytes of a column in three dwords (16 bytes per
//                          column), so that the SAD of one column of the window -- 11 absolute differences -- is three
//                          v_sad_u8 on one broadcast LDS read of the left column x and one read of the right column
//                          x - d (ds_read_b96), which neighbouring lanes take from neighbouring entries.  A wave walks along x: the
//                          window's cost is the running sum of its last 11 column SADs (a ring in registers; the walk is
//                          unrolled by 11 so that the ring's index is a constant), one addition and one subtraction per
//                          (pixel, disparity) where k_stereo_depth spends 33 v_sad_u8 on 44 LDS dwords.  Per pixel the keys
//                          cost << 11 | d of the lanes with d <= d_hi(u) = min(d_max, u - R) -- a per-pixel mask, the walk itself
//                          never looks at the edge -- are reduced as in k_stereo_depth (two minima in the DPP network, the
//                          parabola's neighbours by readlane); every branch on a status is wave-uniform.  The same keys
//                          go, by ds_min_u32, into the workgroup's piece of the right disparity map at column u - d
//                          (neighbouring lanes, neighbouring words) and from there with one global atomic minimum per
//                          column into the row's map: C'(d') = C(v, xr + d', d'), so the left-right search needs no cost of
//                          its own.  Writes the status of steps 1 to 5 and d*, C(d* - 1), C(d*), C(d* + 1) per pixel.
//   k_stereo_dense_finish  lanes over pixels: step 6 from the right map, steps 7 and 8, the three planes.
// The walk starts 10 columns before a wave's first pixel (16 % more column SADs at 64 columns per wave); a row is staged
// once per output row (its bytes come from L2 eleven times), which costs about 200 of a lane's 2 000 to 8 000 instructions.
constexpr int DT_W = 256;                                   // output columns of a workgroup
constexpr int DT_L = DT_W + 2 * SR;                         // staged columns of the left eye
constexpr int DT_R = DT_L + RELOC_STEREO_NUM_DISP_MAX;      // ... of the right eye, and words of the right map's piece
static_assert(STEREO_PASSES * 64 == RELOC_STEREO_NUM_DISP_MAX, "a lane holds num_disparities / 64 disparities");

// the bytes of column x, rows v - R .. v + R, in three dwords (row v - R in the low byte of .x)
__device__ __forceinline__ uint4 stereo_pack_column(const uint8_t *__restrict__ img, int stride, int v, int x)
{
    const uint8_t *p = img + (size_t)(v - SR) * stride + x;
    uint32_t r[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < SP; ++j) r[j >> 2] |= (uint32_t)p[(size_t)j * stride] << (8 * (j & 3));
    return make_uint4(r[0], r[1], r[2], 0u);
}

// the cost of disparity dmin + i from the lane that holds it (i is wave-uniform): a readlane per register, then a choice
// between scalars, which keeps the costs in registers
template <int NP>
__device__ __forceinline__ int stereo_cost_of(const int (&cost)[NP], int i)
{
    int r = __builtin_amdgcn_readlane(cost[0], i & 63);
#pragma unroll
    for (int q = 1; q < NP; ++q) {
        const int t = __builtin_amdgcn_readlane(cost[q], i & 63);
        r = (i >> 6) == q ? t : r;
    }
    return r;
}

// What steps 2 to 5 hand to k_stereo_dense_finish per pixel: d*, C(d* - 1), C(d*), C(d* + 1).  The SAD costs are below 2^15 and
// travel in 16-bit fields of a uint2; the sums of the semi-global pass are below 2^19 and take a uint4.
__device__ __forceinline__ void stereo_best_store(uint2 *o, int dstar, int a, int b, int c)
{
    *o = make_uint2((unsigned)dstar | ((unsigned)b << 16), (unsigned)a | ((unsigned)c << 16));
}
__device__ __forceinline__ void stereo_best_store(uint4 *o, int dstar, int a, int b, int c)
{
    *o = make_uint4((unsigned)dstar, (unsigned)b, (unsigned)a, (unsigned)c);
}
__device__ __forceinline__ void stereo_best_load(const uint2 &t, int &dstar, int &a, int &b, int &c)
{
    dstar = (int)(t.x & 0xFFFFu); b = (int)(t.x >> 16); a = (int)(t.y & 0xFFFFu); c = (int)(t.y >> 16);
}
__device__ __forceinline__ void stereo_best_load(const uint4 &t, int &dstar, int &a, int &b, int &c)
{
    dstar = (int)t.x; b = (int)t.y; a = (int)t.z; c = (int)t.w;
}

// Steps 2 to 5 of pixel (u, v), pixel i of the planes, by its wave: cost[q] is the cost of d = dmin + 64 q + lane, whatever it
// holds beyond d_hi(u).  The keys cost << 11 | d of the lanes inside D go into the workgroup's piece s_dr of the right map
// (first column rb).  The costs are C of k_stereo_dense or the sums S of k_sgm_select, below 2^19 either way.
template <int NP, typename Best>
__device__ __forceinline__ void stereo_select_pixel(const int (&cost)[NP], const StereoParams &p, int u, int lane, unsigned *s_dr, int rb,
                                                    size_t i, Best *__restrict__ o_best, uint8_t *__restrict__ o_status)
{
    const int dmin = p.min_disp, dmax = dmin + p.num_disp - 1;
    const int dhi = min(dmax, u - SR);
    unsigned key = KEY_NONE;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int d = dmin + 64 * q + lane;
        if (d <= dhi) {
            const unsigned kq = ((unsigned)cost[q] << 11) | (unsigned)d;
            key = min(key, kq);
            if (p.lr) atomicMin(&s_dr[u - d - rb], kq);
        }
    }
    int status = RELOC_STEREO_OK, dstar = 0, a = 0, b = 0, c = 0;
    if (dhi - dmin + 1 < 3) status = RELOC_STEREO_RANGE;
    else {
        key = wave_min_u32(key);
        dstar = (int)(key & 0x7FFu);
        b = (int)(key >> 11);
        if (dstar == dmin || dstar == dhi) status = RELOC_STEREO_EDGE;
        else {
            unsigned key2 = KEY_NONE;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const int d = dmin + 64 * q + lane;
                if (d <= dhi && abs(d - dstar) >= 2) key2 = min(key2, ((unsigned)cost[q] << 11) | (unsigned)d);
            }
            key2 = wave_min_u32(key2);
            if (key2 != KEY_NONE && (int)(key2 >> 11) * (100 - p.uniq) <= b * 100) status = RELOC_STEREO_UNIQUENESS;
            else {
                a = stereo_cost_of<NP>(cost, dstar - 1 - dmin);
                c = stereo_cost_of<NP>(cost, dstar + 1 - dmin);
            }
        }
    }
    if (lane == 0) {
        o_status[i] = (uint8_t)status;
        stereo_best_store(o_best + i, dstar, a, b, c);
    }
}

// VOL: the volume pass of the semi-global matcher -- the same walk, but a pixel's costs go to vol[(v w + u) nd + k], k = d - dmin,
// as uint16 (SGM_NONE beyond d_hi(u)) and nothing else is written: selection, right map and statuses follow from the sums.
template <int NP, bool VOL>
__global__ __launch_bounds__(256) void k_stereo_dense(const uint8_t *__restrict__ left, int lstride, const uint8_t *__restrict__ right,
                                                      int rstride, StereoParams p, uint32_t *__restrict__ rmap,
                                                      uint2 *__restrict__ o_best, uint8_t *__restrict__ o_status,
                                                      uint16_t *__restrict__ vol)
{
    __shared__ uint4 s_l[DT_L];
    __shared__ uint4 s_r[DT_R];
    __shared__ unsigned s_dr[DT_R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = p.w, v = blockIdx.y, U0 = blockIdx.x * DT_W, U1 = min(U0 + DT_W, w);
    const int ulo = max(U0, SR), uhi = min(U1, w - SR);              // the workgroup's pixels that pass step 1: ulo <= u < uhi
    const size_t row = (size_t)v * w;
    if (v < SR || v >= p.h - SR || ulo >= uhi) {                      // workgroup-uniform
        if (!VOL)
            for (int u = U0 + tid; u < U1; u += 256) o_status[row + u] = RELOC_STEREO_BORDER;
        return;
    }
    const int dmin = p.min_disp;
    // staged columns: the left eye's xlo .. xlo + nl - 1 (all inside the row), the right eye's rb .. rb + nr - 1, which the
    // lanes of the last disparities reach; a column left of the image is 0 and is not fetched
    const int xlo = ulo - SR, nl = uhi - ulo + 2 * SR;
    const int rb = xlo - dmin - 64 * NP + 1, nr = nl + 64 * NP - 1;
    for (int e = tid; e < nl; e += 256) s_l[e] = stereo_pack_column(left, lstride, v, xlo + e);
    for (int e = tid; e < nr; e += 256) {
        const int x = rb + e;
        s_r[e] = x >= 0 ? stereo_pack_column(right, rstride, v, x) : make_uint4(0u, 0u, 0u, 0u);
        s_dr[e] = KEY_NONE;
    }
    __syncthreads();
    const int S0 = U0 + 64 * wave;
    const int wlo = max(S0, SR), whi = min(S0 + 64, uhi);             // the wave's pixels
    if (!VOL && S0 + lane < U1 && (S0 + lane < SR || S0 + lane >= w - SR)) o_status[row + S0 + lane] = RELOC_STEREO_BORDER;
    if (wlo < whi) {                                                  // wave-uniform
        int ring[NP][SP], cost[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            cost[q] = 0;
#pragma unroll
            for (int k = 0; k < SP; ++k) ring[q][k] = 0;
        }
        const int xend = whi + SR;
        const int ebase = 64 * NP - 1 - lane - xlo;                  // entry of column x - d of chunk q: x + ebase - 64 q
        for (int x0 = wlo - SR; x0 < xend; x0 += SP) {
#pragma unroll
            for (int k = 0; k < SP; ++k) {
                const int x = x0 + k, u = x - SR;
                if (x < xend) {
                    const uint4 lc = s_l[x - xlo];
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        const uint4 rc = s_r[x + ebase - 64 * q];
                        unsigned cs = __builtin_amdgcn_sad_u8(lc.x, rc.x, 0u);
                        cs = __builtin_amdgcn_sad_u8(lc.y, rc.y, cs);
                        cs = __builtin_amdgcn_sad_u8(lc.z, rc.z, cs);
                        cost[q] += (int)cs - ring[q][k];
                        ring[q][k] = (int)cs;
                    }
                    if (u >= wlo) {
                        // ---- cost[q] = C(d) of d = dmin + 64 q + lane: steps 2-5 of pixel (u, v), or its line of the volume ----
                        if constexpr (VOL) {
                            uint16_t *line = vol + (row + u) * (size_t)p.num_disp;
#pragma unroll
                            for (int q = 0; q < NP; ++q)
                                if (64 * q + lane < p.num_disp) line[64 * q + lane] = dmin + 64 * q + lane <= u - SR ? (uint16_t)cost[q] : SGM_NONE;
                        } else stereo_select_pixel<NP>(cost, p, u, lane, s_dr, rb, row + u, o_best, o_status);
                    }
                }
            }
        }
    }
    if (VOL || !p.lr) return;
    __syncthreads();
    // the workgroup's piece of the row's right map: column rb + e; a key exists only where 0 <= R <= rb + e < w
    for (int e = tid; e < nr; e += 256) {
        const unsigned k = s_dr[e];
        if (k != KEY_NONE) atomicMin(&rmap[row + rb + e], k);
    }
}

// pixel i of the w x h planes: step 6 from the right map, steps 7 and 8; Best: uint2 (SAD costs) or uint4 (semi-global sums)
template <typename Best>
__global__ __launch_bounds__(256) void k_stereo_dense_finish(StereoParams p, const uint32_t *__restrict__ rmap,
                                                             const Best *__restrict__ best, uint8_t *__restrict__ status,
                                                             uint16_t *__restrict__ o_mm, float *__restrict__ o_disp)
{
    const int64_t n = (int64_t)p.w * p.h, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int st = status[i];
    uint16_t mm_out = 0;
    float disp_out = 0.f;
    if (st == RELOC_STEREO_OK) {
        int dstar, a, b, c;
        stereo_best_load(best[i], dstar, a, b, c);
        if (p.lr && abs((int)(rmap[i - dstar] & 0x7FFu) - dstar) > 1) st = RELOC_STEREO_LR;
        else {
            const int den = a + c - 2 * b;
            const float delta = den <= 0 ? 0.f : __fdiv_rn((float)(a - c), (float)(2 * den));
            const float disp = __fadd_rn((float)dstar, delta);
            const double z = __ddiv_rn(__dmul_rn(p.fx, p.baseline), (double)disp);
            const double mm = rint(__dmul_rn(z, 1000.0));
            if (mm > 65535.0) st = RELOC_STEREO_FAR;
            else { mm_out = (uint16_t)mm; disp_out = disp; }
        }
        if (st != RELOC_STEREO_OK) status[i] = (uint8_t)st;
    }
    o_mm[i] = mm_out;
    o_disp[i] = disp_out;
}

// the context's dense block, on its first dense call; a failure leaves the context without one
static int stereo_dense_alloc(reloc_ctx *ctx)
{
    StereoState::Dense &d = ctx->stereo.dense;
    if (d.block.p) return RELOC_OK;
    return d.block.layout(ctx, [&](BlockCarver &c) { stereo_dense_lines(c, d, (int64_t)ctx->max_w * ctx->max_h); });
}

// both kernels on ctx's stream, into ctx's dense planes (dense rows of p.w); the planes of the eyes are device pointers;
// speckle: then the speckle stage with ctx's setting ("STEREO, speckle"), inside the same stopwatch bracket
static int stereo_dense_launch(reloc_ctx *ctx, const uint8_t *left, int lstride, const uint8_t *right, int rstride, const StereoParams &p,
                               bool speckle)
{
    StereoState::Dense &d = ctx->stereo.dense;
    const int64_t px = (int64_t)p.w * p.h;
    const int np = (p.num_disp + 63) / 64;
    auto kern = np == 1 ? k_stereo_dense<1, false> : np == 2 ? k_stereo_dense<2, false> : np == 3 ? k_stereo_dense<3, false> : k_stereo_dense<4, false>;
    reloc_prof_begin(ctx, RELOC_PROF_STEREO_DENSE);
    const hipError_t reset = p.lr ? hipMemsetAsync(d.rmap, 0xFF, (size_t)px * 4, ctx->stream) : hipSuccess;      // KEY_NONE
    hipLaunchKernelGGL(kern, dim3((p.w + DT_W - 1) / DT_W, p.h), dim3(256), 0, ctx->stream, left, lstride, right, rstride, p, d.rmap,
                       d.best, d.status, (uint16_t *)nullptr);
    hipLaunchKernelGGL(k_stereo_dense_finish<uint2>, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, ctx->stream, p, d.rmap, d.best,
                       d.status, d.mm, d.disp);
    const int filtered = speckle ? stereo_speckle_launch(ctx, p.w, p.h) : (int)RELOC_OK;
    reloc_prof_end(ctx, RELOC_PROF_STEREO_DENSE);
    HIP_TRY(reset);
    HIP_TRY(hipGetLastError());
    if (filtered) return filtered;
    d.w = p.w; d.h = p.h;
    return RELOC_OK;
}

// ---------------------------------------------------------------------------------------------------
// Semi-global aggregation behind the SAD cost volume (include/reloc_spec.h, "STEREO, semi-global").  Four kernels between the
// staging of k_stereo_dense and k_stereo_dense_finish:
//   k_stereo_dense<NP, true>  the volume pass: C as uint16, the nd costs of a pixel contiguous (2 nd bytes per pixel).
//   k_sgm_paths<NP>           one wave per line of one direction, every selected direction in one launch (blockIdx.y).  A line
//                             starts at a domain pixel whose predecessor lies outside the domain; the wave computes start and
//                             length from its line index (sgm_line) and walks it.  Lanes over disparities, NP per lane as in the
//                             dense kernel; L_r of the previous pixel stays in registers.  Per step: the pixel's cost line (one
//                             read of 2 nd bytes, those of the next SGM_AHEAD pixels already in flight), L_r(q, d - 1) and L_r(q, d + 1) from the
//                             neighbouring lanes by wavefront shifts in the DPP network (across the register boundary by
//                             readlane), the minimum over d for the next step by wave_min_u32, and one integer atomic add per
//                             (pixel, disparity) into S.  Integer addition commutes, so S does not depend on the order in which
//                             the directions arrive, and all of them run side by side: a line is a chain of up to w dependent
//                             steps, and eight directions' worth of waves hide each other's latency where one would not.
//   k_sgm_select<NP>          the tile of k_stereo_dense, a wave over 64 pixels of a row: a pixel's sums (4 nd bytes) into the
//                             registers that held its costs, then the same stereo_select_pixel -- two minima, the right map
//                             keys S << 11 | d (S < 2^19) -- into a uint4 best plane.
//   k_sgm_tap                 the parity tap: S with 0xFFFFFFFF at undefined entries.
// Every offset into the volumes is 64-bit: w h nd passes 2^31 bytes at the capacity limits.
constexpr int SGM_AHEAD = 8;                  // cost lines a path wave keeps in flight ahead of its step
constexpr unsigned SGM_BIG = 1u << 24;        // L_r of a disparity outside D: no sum of penalties brings it near a real cost
static_assert(RELOC_STEREO_SGM_P2_MAX < (1 << 13) && 8 * (SP * SP * 255 + RELOC_STEREO_SGM_P2_MAX) < (1 << 19),
              "S << 11 | disparity is a 30-bit key");

struct SgmLine { int u, v, len; };

// line i of direction (du, dv) over the domain ulo <= u < ulo + dw, vlo <= v < vlo + dh; sgm_line_count of them
__host__ __device__ inline int sgm_line_count(int du, int dv, int dw, int dh) { return dv == 0 ? dh : du == 0 ? dw : dw + dh - 1; }
__host__ __device__ inline SgmLine sgm_line(int i, int du, int dv, int ulo, int vlo, int dw, int dh)
{
    const int ufirst = du > 0 ? ulo : ulo + dw - 1, vfirst = dv > 0 ? vlo : vlo + dh - 1;      // where a walk along +du, +dv enters
    SgmLine l;
    if (dv == 0) { l.u = ufirst; l.v = vlo + i; }
    else if (du == 0 || i < dw) { l.u = ulo + i; l.v = vfirst; }
    else { l.u = ufirst; l.v = vfirst + dv * (i - dw + 1); }
    const int nu = du > 0 ? ulo + dw - l.u : du < 0 ? l.u - ulo + 1 : dh, nv = dv > 0 ? vlo + dh - l.v : dv < 0 ? l.v - vlo + 1 : dw;
    l.len = nu < nv ? nu : nv;
    return l;
}

template <int NP>
__global__ __launch_bounds__(64) void k_sgm_paths(const uint16_t *__restrict__ vol, uint32_t *__restrict__ sum, StereoParams p, int mask,
                                                  unsigned P1, unsigned P2)
{
    const int lane = threadIdx.x, nd = p.num_disp, dmin = p.min_disp;
    int bit = 0;
    for (int k = blockIdx.y; bit < 8; ++bit)                         // the blockIdx.y-th set bit of the mask
        if ((mask >> bit & 1) && k-- == 0) break;
    const int du = bit == 2 || bit == 3 ? 0 : (bit == 0 || bit == 4 || bit == 6) ? 1 : -1;
    const int dv = bit < 2 ? 0 : (bit == 2 || bit == 4 || bit == 7) ? 1 : -1;
    const int ulo = SR + dmin, dw = p.w - SR - ulo, dh = p.h - 2 * SR;
    if ((int)blockIdx.x >= sgm_line_count(du, dv, dw, dh)) return;
    const SgmLine line = sgm_line(blockIdx.x, du, dv, ulo, SR, dw, dh);
    const int64_t step = ((int64_t)dv * p.w + du) * nd;
    int64_t off = ((int64_t)line.v * p.w + line.u) * nd + lane;
    // the cost lines of the next SGM_AHEAD pixels are in flight while a step computes: a step is a short dependent chain
    // (two shifts, four minima, one wave reduction), a line from HBM takes ten times as long
    unsigned ahead[SGM_AHEAD][NP], L[NP], m = 0;
#pragma unroll
    for (int k = 0; k < SGM_AHEAD; ++k)
#pragma unroll
        for (int q = 0; q < NP; ++q) ahead[k][q] = k < line.len && 64 * q + lane < nd ? vol[off + k * step + 64 * q] : SGM_NONE;
#pragma unroll
    for (int q = 0; q < NP; ++q) L[q] = SGM_BIG;
    for (int n0 = 0; n0 < line.len; n0 += SGM_AHEAD) {
#pragma unroll
        for (int k = 0; k < SGM_AHEAD; ++k) {                       // unrolled: the ring's index is a constant
            const int n = n0 + k;
            if (n >= line.len) break;                                // wave-uniform
            unsigned c[NP], Ln[NP], best = SGM_BIG;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                c[q] = ahead[k][q];
                ahead[k][q] = n + SGM_AHEAD < line.len && 64 * q + lane < nd ? vol[off + SGM_AHEAD * step + 64 * q] : SGM_NONE;
            }
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                // L_r(q, d - 1) and L_r(q, d + 1): the neighbouring lanes; lane 0 and lane 63 keep `old`, the neighbouring register's end
                const unsigned below = q ? (unsigned)__builtin_amdgcn_readlane((int)L[q - 1], 63) : SGM_BIG;
                const unsigned above = q + 1 < NP ? (unsigned)__builtin_amdgcn_readlane((int)L[q + 1], 0) : SGM_BIG;
                const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)below, (int)L[q], 0x138, 0xF, 0xF, false);      // wave_shr:1
                const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)above, (int)L[q], 0x130, 0xF, 0xF, false);      // wave_shl:1
                const unsigned inner = min(min(L[q], min(lo, hi) + P1), m + P2) - m;
                Ln[q] = c[q] == SGM_NONE ? SGM_BIG : n ? c[q] + inner : c[q];
                best = min(best, Ln[q]);
            }
            m = wave_min_u32(best);
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                if (Ln[q] != SGM_BIG) atomicAdd(sum + off + 64 * q, Ln[q]);
                L[q] = Ln[q];
            }
            off += step;
        }
    }
}

template <int NP>
__global__ __launch_bounds__(256) void k_sgm_select(const uint32_t *__restrict__ sum, StereoParams p, uint32_t *__restrict__ rmap,
                                                    uint4 *__restrict__ o_best, uint8_t *__restrict__ o_status)
{
    __shared__ unsigned s_dr[DT_R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = p.w, v = blockIdx.y, U0 = blockIdx.x * DT_W, U1 = min(U0 + DT_W, w), nd = p.num_disp;
    const int ulo = max(U0, SR), uhi = min(U1, w - SR);
    const size_t row = (size_t)v * w;
    if (v < SR || v >= p.h - SR || ulo >= uhi) {                      // workgroup-uniform
        for (int u = U0 + tid; u < U1; u += 256) o_status[row + u] = RELOC_STEREO_BORDER;
        return;
    }
    // the workgroup's piece of the right map, the columns of k_stereo_dense's
    const int rb = ulo - SR - p.min_disp - 64 * NP + 1, nr = uhi - ulo + 2 * SR + 64 * NP - 1;
    for (int e = tid; e < nr; e += 256) s_dr[e] = KEY_NONE;
    __syncthreads();
    const int S0 = U0 + 64 * wave;
    const int wlo = max(S0, SR), whi = min(S0 + 64, uhi);             // the wave's pixels
    if (S0 + lane < U1 && (S0 + lane < SR || S0 + lane >= w - SR)) o_status[row + S0 + lane] = RELOC_STEREO_BORDER;
    if (wlo < whi) {                                                  // wave-uniform
        const uint32_t *line = sum + (row + wlo) * (size_t)nd + lane;
        int cost[NP], next[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) cost[q] = 64 * q + lane < nd ? (int)line[64 * q] : 0;
        for (int u = wlo; u < whi; ++u, line += nd) {
#pragma unroll
            for (int q = 0; q < NP; ++q) next[q] = u + 1 < whi && 64 * q + lane < nd ? (int)line[nd + 64 * q] : 0;
            stereo_select_pixel<NP>(cost, p, u, lane, s_dr, rb, row + u, o_best, o_status);
#pragma unroll
            for (int q = 0; q < NP; ++q) cost[q] = next[q];
        }
    }
    if (!p.lr) return;
    __syncthreads();
    for (int e = tid; e < nr; e += 256) {
        const unsigned k = s_dr[e];
        if (k != KEY_NONE) atomicMin(&rmap[row + rb + e], k);
    }
}

// entry i of [v][u][k]: the sum where (u, v, dmin + k) is defined, 0xFFFFFFFF elsewhere
__global__ __launch_bounds__(256) void k_sgm_tap(const uint32_t *__restrict__ sum, int w, int h, int nd, int dmin, uint32_t *__restrict__ out)
{
    const int64_t n = (int64_t)w * h * nd, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = (int)(i % nd), u = (int)(i / nd % w), v = (int)(i / nd / w);
    const bool defined = v >= SR && v < h - SR && u >= SR && u < w - SR && dmin + k <= u - SR;
    out[i] = defined ? sum[i] : 0xFFFFFFFFu;
}

// the context's semi-global block on its first such pass, sized from that pass; grown only when a later pass needs more
static int stereo_sgm_alloc(reloc_ctx *ctx, int w, int h, int nd)
{
    StereoState::Sgm &g = ctx->stereo.sgm;
    const int64_t px = (int64_t)w * h, entries = px * nd;
    if (g.block.p && entries <= g.cap_entries && px <= g.cap_px) return RELOC_OK;
    const int64_t ne = entries > g.cap_entries ? entries : g.cap_entries, npx = px > g.cap_px ? px : g.cap_px;
    BlockCarver need;
    stereo_sgm_lines(need, g, ne, npx);
    if (g.block.reserve(ctx, need.at)) {       // the old block, its pointers and the last pass stay as they were
        reloc_set_error("stereo sgm: no device memory for the volumes of a %d x %d pass over %d disparities (%zu bytes)", w, h, nd, need.at);
        return RELOC_E_CAPACITY;
    }
    BlockCarver commit{g.block.p};
    stereo_sgm_lines(commit, g, ne, npx);
    g.cap_entries = ne; g.cap_px = npx;
    g.w = g.h = 0;                             // a grown block holds no pass
    return RELOC_OK;
}

static int stereo_sgm_args_check(int path_mask, int p1, int p2)
{
    if (path_mask < 1 || path_mask > 255) { reloc_set_error("bad argument: stereo sgm path_mask %d outside 1..255", path_mask); return RELOC_E_ARG; }
    if (p1 < 0 || p2 < p1 || p2 > RELOC_STEREO_SGM_P2_MAX) {
        reloc_set_error("bad argument: stereo sgm penalties p1 %d, p2 %d outside 0 <= p1 <= p2 <= %d", p1, p2, RELOC_STEREO_SGM_P2_MAX);
        return RELOC_E_ARG;
    }
    return RELOC_OK;
}

// the semi-global pass on ctx's stream into ctx's dense planes, the twin of stereo_dense_launch
static int stereo_sgm_launch(reloc_ctx *ctx, const uint8_t *left, int lstride, const uint8_t *right, int rstride, const StereoParams &p,
                             int mask, int p1, int p2, bool speckle)
{
    if (int rc = stereo_sgm_alloc(ctx, p.w, p.h, p.num_disp)) return rc;
    StereoState::Dense &d = ctx->stereo.dense;
    StereoState::Sgm &g = ctx->stereo.sgm;
    const int64_t px = (int64_t)p.w * p.h;
    const int np = (p.num_disp + 63) / 64, dw = p.w - 2 * SR - p.min_disp, dh = p.h - 2 * SR;
    const int ndirs = __builtin_popcount((unsigned)mask), diagonal = mask & 0xF0, lines = diagonal ? dw + dh - 1 : dw > dh ? dw : dh;
    auto vol = np == 1 ? k_stereo_dense<1, true> : np == 2 ? k_stereo_dense<2, true> : np == 3 ? k_stereo_dense<3, true> : k_stereo_dense<4, true>;
    auto paths = np == 1 ? k_sgm_paths<1> : np == 2 ? k_sgm_paths<2> : np == 3 ? k_sgm_paths<3> : k_sgm_paths<4>;
    auto select = np == 1 ? k_sgm_select<1> : np == 2 ? k_sgm_select<2> : np == 3 ? k_sgm_select<3> : k_sgm_select<4>;
    const dim3 tiles((p.w + DT_W - 1) / DT_W, p.h);
    reloc_prof_begin(ctx, RELOC_PROF_STEREO_SGM);
    hipError_t reset = hipMemsetAsync(g.sum, 0, (size_t)(px * p.num_disp) * 4, ctx->stream);
    if (reset == hipSuccess && p.lr) reset = hipMemsetAsync(d.rmap, 0xFF, (size_t)px * 4, ctx->stream);      // KEY_NONE
    hipLaunchKernelGGL(vol, tiles, dim3(256), 0, ctx->stream, left, lstride, right, rstride, p, (uint32_t *)nullptr, (uint2 *)nullptr,
                       (uint8_t *)nullptr, g.vol);
    if (dw > 0)                                                       // else no pixel has a disparity to search: the domain is empty
        hipLaunchKernelGGL(paths, dim3(lines, ndirs), dim3(64), 0, ctx->stream, g.vol, g.sum, p, mask, (unsigned)p1, (unsigned)p2);
    hipLaunchKernelGGL(select, tiles, dim3(256), 0, ctx->stream, g.sum, p, d.rmap, g.best, d.status);
    hipLaunchKernelGGL(k_stereo_dense_finish<uint4>, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, ctx->stream, p, d.rmap, g.best,
                       d.status, d.mm, d.disp);
    const int filtered = speckle ? stereo_speckle_launch(ctx, p.w, p.h) : (int)RELOC_OK;
    reloc_prof_end(ctx, RELOC_PROF_STEREO_SGM);
    HIP_TRY(reset);
    HIP_TRY(hipGetLastError());
    if (filtered) return filtered;
    d.w = g.w = p.w; d.h = g.h = p.h;
    g.nd = p.num_disp; g.dmin = p.min_disp;
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
    if (int rc = stereo_sgm_args_check(0xFF, p1, p2)) return rc;
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

RELOC_API int reloc_stereo_sgm_image(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, double fx,
                                     double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check,
                                     int path_mask, int p1, int p2, uint16_t *depth_mm, float *disparity, uint8_t *status)
{
    ARG_CHECK_CTX(ctx, left && right && depth_mm && w >= SP && h >= SP && stride >= w, "reloc_stereo_sgm_image");
    if (!(fx - fx == 0.0) || fx <= 0.0) { reloc_set_error("bad argument: stereo fx %g is not finite and > 0", fx); return RELOC_E_ARG; }
    if (int rc = stereo_args_check(baseline_m, min_disparity, num_disparities, uniqueness, lr_check, false)) return rc;
    if (int rc = stereo_sgm_args_check(path_mask, p1, p2)) return rc;
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    if (int rc = stereo_dense_alloc(ctx)) return rc;
    if (int rc = stereo_sgm_alloc(ctx, w, h, num_disparities)) return rc;
    const StereoState::Dense &d = ctx->stereo.dense;
    const int64_t bytes = (int64_t)(h - 1) * stride + w, px = (int64_t)w * h;
    HostStaging st{ctx};
    uint8_t *dl = st.slot<uint8_t>(0, bytes), *dr = st.slot<uint8_t>(1, bytes);
    if (st.rc) return st.finish();
    st.upload(dl, left, bytes);
    st.upload(dr, right, bytes);
    const StereoParams p = {fx, baseline_m, w, h, min_disparity, num_disparities, uniqueness, lr_check};
    st.run([&] { return stereo_sgm_launch(ctx, dl, stride, dr, stride, p, path_mask, p1, p2, false); });
    st.download(depth_mm, d.mm, px * 2);
    if (disparity) st.download(disparity, d.disp, px * 4);
    if (status) st.download(status, d.status, px);
    return st.finish();
}

RELOC_API int reloc_stereo_sgm_debug(reloc_ctx *ctx, uint32_t *S, int32_t *w, int32_t *h, int32_t *nd)
{
    ARG_CHECK_CTX(ctx, true, "reloc_stereo_sgm_debug");
    const StereoState::Sgm &g = ctx->stereo.sgm;
    if (!g.block.p || g.w == 0) { reloc_set_error("no semi-global stereo pass on this context yet"); return RELOC_E_STATE; }
    const int64_t n = (int64_t)g.w * g.h * g.nd;
    HostStaging st{ctx};
    if (S) {
        uint32_t *out = st.slot<uint32_t>(0, n);
        if (st.rc) return st.finish();
        st.launch(k_sgm_tap, dim3((unsigned)((n + 255) / 256)), dim3(256), (const uint32_t *)g.sum, g.w, g.h, g.nd, g.dmin, out);
        st.download(S, out, n * 4);
    }
    if (int rc = st.finish()) return rc;
    if (w) *w = g.w;
    if (h) *h = g.h;
    if (nd) *nd = g.nd;
    return RELOC_OK;
}

RELOC_API int reloc_stereo_depth_image(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, double fx,
                                       double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check,
                                       uint16_t *depth_mm, float *disparity, uint8_t *status)
{
    ARG_CHECK_CTX(ctx, left && right && depth_mm && w >= SP && h >= SP && stride >= w, "reloc_stereo_depth_image");
    if (!(fx - fx == 0.0) || fx <= 0.0) { reloc_set_error("bad argument: stereo fx %g is not finite and > 0", fx); return RELOC_E_ARG; }
    if (int rc = stereo_args_check(baseline_m, min_disparity, num_disparities, uniqueness, lr_check, false)) return rc;
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    if (int rc = stereo_dense_alloc(ctx)) return rc;
    const StereoState::Dense &d = ctx->stereo.dense;
    const int64_t bytes = (int64_t)(h - 1) * stride + w, px = (int64_t)w * h;
    HostStaging st{ctx};
    uint8_t *dl = st.slot<uint8_t>(0, bytes), *dr = st.slot<uint8_t>(1, bytes);
    if (st.rc) return st.finish();
    st.upload(dl, left, bytes);
    st.upload(dr, right, bytes);
    const StereoParams p = {fx, baseline_m, w, h, min_disparity, num_disparities, uniqueness, lr_check};
    st.run([&] { return stereo_dense_launch(ctx, dl, stride, dr, stride, p, false); });
    st.download(depth_mm, d.mm, px * 2);
    if (disparity) st.download(disparity, d.disp, px * 4);
    if (status) st.download(status, d.status, px);
    return st.finish();
}

int stereo_dense_frame(reloc_ctx *ctx, reloc_ctx *right, int w, int h, int order, int *ww, int *wh)
{
    StereoState &s = ctx->stereo;
    if (int rc = stereo_pair_check(ctx, right, w, h, ww, wh)) return rc;
    if (int rc = stereo_dense_alloc(ctx)) return rc;
    const uint8_t *plane[2];
    int pstride[2];
    if (int rc = stereo_gray_planes(ctx, right, ctx->frame_img, right->frame_img, w, h, *ww, *wh, order, plane, pstride)) return rc;
    const StereoParams p = {ctx->cam.K4[0], s.baseline, *ww, *wh, s.min_disp, s.num_disp, s.uniq, s.lr};
    if (s.sgm_paths)
        return stereo_sgm_launch(ctx, plane[0], pstride[0], plane[1], pstride[1], p, s.sgm_paths == 4 ? 0x0F : 0xFF, s.sgm_p1, s.sgm_p2,
                                 s.speckle_window > 0);
    return stereo_dense_launch(ctx, plane[0], pstride[0], plane[1], pstride[1], p, s.speckle_window > 0);
}

RELOC_API int reloc_stereo_frame_depth(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *img, const uint8_t *img_right, int w, int h,
                                       int order, uint16_t *depth_mm, int32_t *out_w, int32_t *out_h)
{
    ARG_CHECK_CTX(ctx, right && img && img_right && w >= 64 && h >= 64, "reloc_stereo_frame_depth");
    if (int rc = stereo_pair_entry(ctx, right, w, h)) return rc;
    StereoPairStaging st(ctx, right);
    st.upload_pair(img, img_right, w, h);
    int ww = 0, wh = 0;
    st.run([&] { return stereo_dense_frame(ctx, right, w, h, order, &ww, &wh); });
    if (depth_mm) st.download(depth_mm, ctx->stereo.dense.mm, (int64_t)ww * wh * 2);
    if (int rc = st.finish()) return rc;
    if (out_w) *out_w = ww;
    if (out_h) *out_h = wh;
    return RELOC_OK;
}

RELOC_API int reloc_stereo_dense_debug(reloc_ctx *ctx, uint16_t *depth_mm, float *disparity, uint8_t *status, int32_t *w, int32_t *h)
{
    ARG_CHECK_CTX(ctx, true, "reloc_stereo_dense_debug");
    const StereoState::Dense &d = ctx->stereo.dense;
    if (!d.block.p || d.w == 0) { reloc_set_error("no dense stereo pass on this context yet"); return RELOC_E_STATE; }
    const int64_t px = (int64_t)d.w * d.h;
    HostStaging st{ctx};
    if (depth_mm) st.download(depth_mm, d.mm, px * 2);
    if (disparity) st.download(disparity, d.disp, px * 4);
    if (status) st.download(status, d.status, px);
    if (int rc = st.finish()) return rc;
    if (w) *w = d.w;
    if (h) *h = d.h;
    return RELOC_OK;
}
