// reloc_obstacle.hip -- local obstacle perception (include/reloc_spec.h "OBSTACLE"; DESIGN.md "Local obstacles").
// Per depth frame:
//   k_obs_blocks       (d) a workgroup per block: count, minimum and the two-pass float64 variance in a fixed tree, a byte out
//   k_obs_filtered     the filtered image itself, for reloc_obs_filter_depth only: every consumer below reads through the mask
//   k_obs_profile      (a)-(c) a workgroup per 16 adjacent sampled columns: the strip's rows staged in LDS as uint32 keys (a valid
//                      depth is a positive float, so its bits order as it does; an invalid pixel is the largest key), rows
//                      read 16 pixels at a time, four rows per wave; then a wave per column, a radix select over ballots for
//                      s[lo_i] and a minimum for s[hi_i]: a selection, no sort
// Per grid update, one launch:
//   k_obs_grid_update  (e) the columns' contributions as cell indices in LDS, five per column in the rule's order; every output
//                      cell reads its shifted source or zero, decays it and walks the list in order: the sums are those of the
//                      serial loop by construction, no atomics.  Reads grid[cur], writes the other one.
// Per query:
//   k_obs_rays         (f) a thread per sector
//   k_obs_readout      (g) one workgroup: the debug image, the count and the maximum
#include "reloc_teach.h"

#include <math.h>

constexpr uint32_t OBS_KEY_NONE = 0xFFFFFFFFu;     // no valid float has these bits (they are a NaN's)
constexpr int OBS_TILE = 16;                        // k_obs_profile: adjacent sampled columns per workgroup; 35 KB of keys at the most

struct ObsSrc { const void *data; int w, h; };
// the block mask of a frame as a consumer reads it; mask == NULL: no filter
struct ObsMask { const uint8_t *mask; int bh, bw, nby, nbx; float fill; };
struct ObsFilterPrm { int bh, bw, min_count, n_cov; float lo, hi; double var_thresh, min_solid; };

// (a) a depth pixel is reloc_teach.h's depth_pixel, at r * w + c of the plane
__device__ __forceinline__ bool obs_valid(float z, float lo, float hi) { return z > lo && z < hi && isfinite(z); }
// the pixel behind the filter: fill inside a traversable block
template <bool F32>
__device__ __forceinline__ float obs_pixel(const ObsSrc &s, const ObsMask &m, int r, int c)
{
    if (m.mask) {
        const int by = r / m.bh, bx = c / m.bw;
        if (by < m.nby && bx < m.nbx && m.mask[by * m.nbx + bx]) return m.fill;
    }
    return depth_pixel(s.data, F32, (size_t)r * s.w + c);
}

// sums of a 256-thread workgroup in a fixed tree; every thread gets the total.  s: 256 doubles
__device__ __forceinline__ double obs_tree_sum(double v, double *s)
{
    __syncthreads();
    s[threadIdx.x] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) s[threadIdx.x] = __dadd_rn(s[threadIdx.x], s[threadIdx.x + k]);
        __syncthreads();
    }
    return s[0];
}

template <bool F32>
__global__ __launch_bounds__(256) void k_obs_blocks(ObsSrc src, ObsFilterPrm p, int nbx, uint8_t *__restrict__ mask)
{
    __shared__ double s_sum[256];
    __shared__ float s_min[256];
    __shared__ int s_n[256];
    const int t = threadIdx.x, by = blockIdx.x / nbx, bx = blockIdx.x % nbx, npix = p.bh * p.bw;
    int n = 0;
    float mn = INFINITY;
    double sum = 0.0;
    for (int i = t; i < npix; i += 256) {
        const float z = depth_pixel(src.data, F32, (size_t)(by * p.bh + i / p.bw) * src.w + bx * p.bw + i % p.bw);
        if (obs_valid(z, p.lo, p.hi)) { ++n; mn = fminf(mn, z); sum = __dadd_rn(sum, (double)z); }
    }
    s_min[t] = mn;
    s_n[t] = n;
    const double total = obs_tree_sum(sum, s_sum);
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) { s_min[t] = fminf(s_min[t], s_min[t + k]); s_n[t] += s_n[t + k]; }
        __syncthreads();
    }
    const int N = s_n[0];
    const double mean = N > 0 ? __ddiv_rn(total, (double)N) : 0.0;
    double ss = 0.0;
    for (int i = t; i < npix; i += 256) {
        const float z = depth_pixel(src.data, F32, (size_t)(by * p.bh + i / p.bw) * src.w + bx * p.bw + i % p.bw);
        if (obs_valid(z, p.lo, p.hi)) { const double d = __dsub_rn((double)z, mean); ss = __dadd_rn(ss, __dmul_rn(d, d)); }
    }
    const double ss_total = obs_tree_sum(ss, s_sum);
    if (t == 0) {
        const double var = N > 0 ? __ddiv_rn(ss_total, (double)N) : 0.0;
        mask[blockIdx.x] = N >= p.min_count && N <= p.n_cov && var > p.var_thresh && (double)s_min[0] > p.min_solid;
    }
}

template <bool F32>
__global__ __launch_bounds__(256) void k_obs_filtered(ObsSrc src, ObsMask m, float *__restrict__ out)
{
    const int n = src.w * src.h;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = obs_pixel<F32>(src, m, i / src.w, i % src.w);
}

// (c) from the two selected values
__device__ __forceinline__ float obs_percentile(uint32_t k_lo, uint32_t k_hi, float g)
{
    const float s_lo = __uint_as_float(k_lo), s_hi = __uint_as_float(k_hi), d = __fsub_rn(s_hi, s_lo);
    return g >= 0.5f ? __fsub_rn(s_hi, __fmul_rn(d, __fsub_rn(1.0f, g))) : __fadd_rn(s_lo, __fmul_rn(d, g));
}

// OBS_TILE adjacent sampled columns per workgroup of eight waves.  Dynamic LDS: the strip, padded to a multiple of 64 rows, as
// rows of OBS_TILE + 1 keys (the odd pitch lets a wave read one column without a bank conflict).  Staged row by row, OBS_TILE
// pixels of a row at a time; then a wave per column, its values in up to eight registers per lane: the count is a ballot, s[lo_i]
// a radix select from the top bit down (32 rounds of ballots: how many of the keys that share the bits decided so far have a 0
// here), s[hi_i] either the same value or the smallest key above it.
template <bool F32>
__global__ __launch_bounds__(512) void k_obs_profile(ObsSrc src, ObsMask m, int step, int ncols, float lo, float hi, float qf, int min_valid,
                                                     float fill, float *__restrict__ prof, int32_t *__restrict__ cnt)
{
    constexpr int PITCH = OBS_TILE + 1, SUBS = 512 / OBS_TILE, REGS = RELOC_OBS_MAX_STRIP / 64;
    extern __shared__ __align__(16) uint32_t s_key[];
    const int r0 = src.h / 3, rows = 2 * src.h / 3 - r0, rows_pad = (rows + 63) & ~63;
    {
        const int lc = threadIdx.x & (OBS_TILE - 1), sub = threadIdx.x / OBS_TILE, col = blockIdx.x * OBS_TILE + lc;
        const int cc = min(col, ncols - 1) * step;      // every thread loads, from a pixel of the strip: no branch around the loads,
#pragma unroll 4                                        // several of them in flight
        for (int r = sub; r < rows_pad; r += SUBS) {
            const float z = obs_pixel<F32>(src, m, r0 + min(r, rows - 1), cc);
            s_key[r * PITCH + lc] = col < ncols && r < rows && obs_valid(z, lo, hi) ? __float_as_uint(z) : OBS_KEY_NONE;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, regs = rows_pad >> 6;
    for (int c = wave; c < OBS_TILE; c += 8) {          // everything below is the same in all lanes of a wave but key[]
        const int col = blockIdx.x * OBS_TILE + c;
        if (col >= ncols) break;
        uint32_t key[REGS];
        int n = 0;
#pragma unroll
        for (int k = 0; k < REGS; ++k) {
            key[k] = k < regs ? s_key[(lane + 64 * k) * PITCH + c] : OBS_KEY_NONE;
            n += __popcll(__ballot(key[k] != OBS_KEY_NONE));
        }
        float out = fill;
        if (n >= min_valid) {                           // min_valid >= 1: there is a value of every rank below n
            const float vi = __fmul_rn((float)(n - 1), qf), lo_f = floorf(vi);
            const int lo_i = (int)lo_f, hi_i = min(lo_i + 1, n - 1);
            uint32_t s_lo = 0, decided = 0;             // the bits of s[lo_i] found so far, and which they are
            int rank = lo_i;                            // its rank among the keys that share them
            for (int bit = 31; bit >= 0; --bit) {
                int zeros = 0;
#pragma unroll
                for (int k = 0; k < REGS; ++k)
                    if (k < regs) zeros += __popcll(__ballot(((key[k] ^ s_lo) & decided) == 0 && !(key[k] >> bit & 1u)));
                if (rank >= zeros) { rank -= zeros; s_lo |= 1u << bit; }
                decided |= 1u << bit;
            }
            int le = 0;                                 // #(x <= s[lo_i]) > lo_i
            uint32_t above = OBS_KEY_NONE;
#pragma unroll
            for (int k = 0; k < REGS; ++k) {
                le += __popcll(__ballot(key[k] <= s_lo));
                above = min(above, key[k] > s_lo ? key[k] : OBS_KEY_NONE);
            }
            const uint32_t s_hi = hi_i < le ? s_lo : wave_min_u32(above);
            out = obs_percentile(s_lo, s_hi, __fsub_rn(vi, lo_f));
        }
        if (lane == 0) { prof[col] = out; cnt[col] = n; }
    }
}

// (e), (f): centre + (int)(dist * c / res), false when that leaves [0, cells)
__device__ __forceinline__ bool obs_cell(double dist, double c, double res, int centre, int cells, int &g)
{
    const double q = __ddiv_rn(__dmul_rn(dist, c), res);
    if (!(fabs(q) < 1.0e9)) return false;               // beyond every grid (and beyond int), or not a number
    g = centre + (int)q;
    return (unsigned)g < (unsigned)cells;
}

__global__ __launch_bounds__(256) void k_obs_grid_update(const float *__restrict__ src, float *__restrict__ dst, int cells, int sx, int sy,
                                                         float decay, const float *__restrict__ prof, const int32_t *__restrict__ cnt,
                                                         const double2 *__restrict__ dirs, int ncols, int min_valid, double res, float hit,
                                                         float hit_nb)
{
    __shared__ int32_t s_list[5 * RELOC_OBS_MAX_GRID_COLS];
    const int centre = cells / 2;
    for (int k = threadIdx.x; k < ncols; k += blockDim.x) {
        int32_t e[5] = {-1, -1, -1, -1, -1};
        if (cnt[k] >= min_valid) {
            const double depth = (double)prof[k];
            const double2 d = dirs[k];
            int gx, gy;
            if (obs_cell(depth, d.x, res, centre, cells, gx) && obs_cell(depth, d.y, res, centre, cells, gy)) {
                e[0] = gy * cells + gx;
                if (gx + 1 < cells) e[1] = e[0] + 1;
                if (gx - 1 >= 0) e[2] = e[0] - 1;
                if (gy + 1 < cells) e[3] = e[0] + cells;
                if (gy - 1 >= 0) e[4] = e[0] - cells;
            }
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) s_list[5 * k + j] = e[j];
    }
    __syncthreads();
    const int n = cells * cells;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += gridDim.x * blockDim.x) {
        const int r = idx / cells + sy, c = idx % cells + sx;                 // |sx|, |sy| <= cells: the host clamps
        float v = (unsigned)r < (unsigned)cells && (unsigned)c < (unsigned)cells ? src[r * cells + c] : 0.0f;
        v = __fmul_rn(v, decay);
        for (int k = 0; k < ncols; ++k) {
            if (s_list[5 * k] == idx) v = __fadd_rn(v, hit);
#pragma unroll
            for (int j = 1; j < 5; ++j)
                if (s_list[5 * k + j] == idx) v = __fadd_rn(v, hit_nb);
        }
        dst[idx] = v;
    }
}

__global__ __launch_bounds__(64) void k_obs_rays(const float *__restrict__ grid, int cells, const double2 *__restrict__ dirs, int n, double res,
                                                 double max_range, float obstacle_hits, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int centre = cells / 2;
    const double2 d = dirs[i];
    double found = max_range;
    for (double dist = __dmul_rn(res, 2.0); dist < max_range; dist = __dadd_rn(dist, res)) {
        int gx, gy;
        if (!(obs_cell(dist, d.x, res, centre, cells, gx) && obs_cell(dist, d.y, res, centre, cells, gy))) break;
        if (grid[gy * cells + gx] >= obstacle_hits) { found = dist; break; }
    }
    out[i] = found;
}

// stats: [0] cells >= obstacle_hits, [1] the bits of the maximum
__global__ __launch_bounds__(1024) void k_obs_readout(const float *__restrict__ grid, int n, float obstacle_hits, uint8_t *__restrict__ image,
                                                      int32_t *__restrict__ stats)
{
    __shared__ int s_n[1024];
    __shared__ float s_max[1024];
    const int t = threadIdx.x;
    int cnt = 0;
    float mx = -INFINITY;
    for (int i = t; i < n; i += 1024) {
        const float v = grid[i];
        cnt += v >= obstacle_hits;
        mx = fmaxf(mx, v);
        const float u = fminf(fmaxf(__fdiv_rn(v, obstacle_hits), 0.0f), 1.0f);
        image[i] = (uint8_t)__fmul_rn(u, 255.0f);
    }
    s_n[t] = cnt;
    s_max[t] = mx;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
        if (t < k) { s_n[t] += s_n[t + k]; s_max[t] = fmaxf(s_max[t], s_max[t + k]); }
        __syncthreads();
    }
    if (t == 0) { stats[0] = s_n[0]; stats[1] = (int32_t)__float_as_uint(s_max[0]); }
}

// One pass of the rectangular erode / dilate of the cv2 shim over 8-bit pixels: the minimum (maximum) of the k pixels from
// anchor columns (HORIZONTAL) or rows before a pixel on, those outside the image left out: they never lower an erosion and never
// raise a dilation.  A k x 1 pass and a 1 x k pass make the rectangle.
template <bool DILATE, bool HORIZONTAL>
__global__ __launch_bounds__(256) void k_morph_pass(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int w, int h, int k, int anchor)
{
    const int n = w * h;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int r = i / w, c = i % w;
        const int at = HORIZONTAL ? c : r, len = HORIZONTAL ? w : h, stride = HORIZONTAL ? 1 : w;
        const int j0 = max(at - anchor, 0), j1 = min(at - anchor + k, len);          // j0 <= at < j1: the anchor lies in the kernel
        const uint8_t *p = src + i + (j0 - at) * stride;
        int v = DILATE ? 0 : 255;
        for (int j = j0; j < j1; ++j, p += stride) v = DILATE ? max(v, (int)*p) : min(v, (int)*p);
        dst[i] = (uint8_t)v;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// the frame block, taken by the first call that reads a depth image
static int obs_frame_alloc(reloc_ctx *ctx)
{
    ObstacleState &o = ctx->obs;
    if (o.frame_block.p) return RELOC_OK;
    const int64_t blocks = (int64_t)ctx->max_w * ctx->max_h / (RELOC_OBS_MIN_BLOCK * RELOC_OBS_MIN_BLOCK) + 1;
    return o.frame_block.layout(ctx, [&](BlockCarver &c) {
        c(o.prof, RELOC_OBS_MAX_COLS);
        c(o.cnt, RELOC_OBS_MAX_COLS);
        c(o.mask, blocks);
    });
}

// a host image on scratch slot 5, or the plane of the last dense stereo pass where it lies (depth == NULL)
struct ObsFrame { ObsSrc src; bool f32; };
static int obs_source(HostStaging &st, const void *depth, int is_f32, int w, int h, bool stereo, const char *who, ObsFrame &f)
{
    reloc_ctx *ctx = st.ctx;
    const StereoState::Dense *d = stereo ? stereo_last_dense(ctx) : nullptr;
    if (stereo && !d) { reloc_set_error("%s: no dense stereo pass on this context yet", who); return RELOC_E_STATE; }
    if (d) { w = d->w; h = d->h; }
    if (w > RELOC_OBS_MAX_COLS || (int64_t)w * h > (int64_t)ctx->max_w * ctx->max_h) {
        reloc_set_error("%s: depth image %d x %d exceeds the capacity (ctx %d x %d, %d columns)", who, w, h, ctx->max_w, ctx->max_h, RELOC_OBS_MAX_COLS);
        return RELOC_E_CAPACITY;
    }
    if (2 * h / 3 - h / 3 > RELOC_OBS_MAX_STRIP) {
        reloc_set_error("%s: a strip of %d rows exceeds the capacity (%d)", who, 2 * h / 3 - h / 3, RELOC_OBS_MAX_STRIP);
        return RELOC_E_CAPACITY;
    }
    if (int rc = obs_frame_alloc(ctx)) return rc;
    const void *dev = d ? (const void *)d->mm : (const void *)st.upload_slot(5, (const uint8_t *)depth, (int64_t)w * h * (is_f32 ? 4 : 2));
    f = ObsFrame{{dev, w, h}, !stereo && is_f32 != 0};
    return st.rc;
}

// the frame's block mask (rule (d)) into o.mask when `filter`; what a consumer reads the frame through
static ObsMask obs_mask(HostStaging &st, const ObsFrame &f, bool filter)
{
    const ObstacleState &o = st.ctx->obs;
    if (!filter) return ObsMask{nullptr, 1, 1, 0, 0, 0.0f};
    const int nby = f.src.h / o.bh, nbx = f.src.w / o.bw;
    const ObsFilterPrm p{o.bh, o.bw, o.min_count, o.n_cov, o.f_lo, o.f_hi, o.var_thresh, o.min_solid};
    if (nby * nbx > 0) st.launch(f.f32 ? k_obs_blocks<true> : k_obs_blocks<false>, dim3(nby * nbx), dim3(256), f.src, p, nbx, o.mask);
    return ObsMask{o.mask, o.bh, o.bw, nby, nbx, o.f_fill};
}

struct ObsProfilePrm { int step; float lo, hi; int q, min_valid; float fill; int use_filter; };

static int obs_profile_check(const reloc_ctx *ctx, const ObsProfilePrm &p, const char *who)
{
    if (!(p.step >= 1 && p.q >= 0 && p.q <= 100 && p.min_valid >= 1 && occ_finite(p.lo) && occ_finite(p.hi) && occ_finite(p.fill) && p.lo >= 0.0f)) {
        reloc_set_error("bad argument: %s: step >= 1, 0 <= lo, q in [0, 100], min_valid >= 1, everything finite", who);
        return RELOC_E_ARG;
    }
    if (p.use_filter && !ctx->obs.filter_on()) { reloc_set_error("%s: the traversability filter is off on this context (reloc_obs_set_filter)", who); return RELOC_E_STATE; }
    return RELOC_OK;
}

// mask (when asked for) and profile of a frame into o.prof / o.cnt; returns the number of columns
static int obs_profile_launch(HostStaging &st, const ObsFrame &f, const ObsProfilePrm &p)
{
    const ObstacleState &o = st.ctx->obs;
    const ObsMask m = obs_mask(st, f, p.use_filter != 0);
    const int ncols = (f.src.w + p.step - 1) / p.step, rows = 2 * f.src.h / 3 - f.src.h / 3;
    const float qf = (float)p.q / 100.0f;
    const size_t lds = (size_t)((rows + 63) & ~63) * (OBS_TILE + 1) * sizeof(uint32_t);
    st.run([&] {
        hipLaunchKernelGGL(f.f32 ? k_obs_profile<true> : k_obs_profile<false>, dim3((ncols + OBS_TILE - 1) / OBS_TILE), dim3(512), lds, st.ctx->stream,
                           f.src, m, p.step, ncols, p.lo, p.hi, qf, p.min_valid, p.fill, o.prof, o.cnt);
        st.hip(hipGetLastError(), "kernel launch");
        return st.rc;
    });
    return ncols;
}

RELOC_API int reloc_obs_set_filter(reloc_ctx *ctx, int bh, int bw, float lo, float hi, int min_count, double coverage, double var_thresh,
                                   double min_solid, float fill)
{
    ARG_CHECK_CTX(ctx, true, "reloc_obs_set_filter");
    ObstacleState &o = ctx->obs;
    if (bh == 0 && bw == 0) { o.bh = o.bw = 0; return RELOC_OK; }
    ARG_CHECK(bh > 0 && bw > 0 && occ_finite(lo) && occ_finite(hi) && lo >= 0.0f && hi > lo && min_count >= 1 && occ_finite(coverage) && coverage > 0.0 &&
                  occ_finite(var_thresh) && occ_finite(min_solid) && occ_finite(fill),
              "reloc_obs_set_filter: positive block sides, 0 <= lo < hi, min_count >= 1, coverage > 0, everything finite");
    if (bh < RELOC_OBS_MIN_BLOCK || bw < RELOC_OBS_MIN_BLOCK || bh > RELOC_OBS_MAX_BLOCK || bw > RELOC_OBS_MAX_BLOCK) {
        reloc_set_error("reloc_obs_set_filter: block %d x %d outside the capacity (sides %d .. %d)", bh, bw, RELOC_OBS_MIN_BLOCK, RELOC_OBS_MAX_BLOCK);
        return RELOC_E_CAPACITY;
    }
    int n_cov = -1;                                     // the largest n with n / (bh * bw) < coverage, as F:43 divides
    for (int n = 0; n <= bh * bw; ++n)
        if ((double)n / (double)(bh * bw) < coverage) n_cov = n;
    o.bh = bh; o.bw = bw; o.f_lo = lo; o.f_hi = hi; o.min_count = min_count; o.n_cov = n_cov;
    o.var_thresh = var_thresh; o.min_solid = min_solid; o.f_fill = fill;
    return RELOC_OK;
}

RELOC_API int reloc_obs_get_filter(reloc_ctx *ctx, int32_t *bh, int32_t *bw, float *lo, float *hi, int32_t *min_count, int32_t *n_cov,
                                   double *var_thresh, double *min_solid, float *fill)
{
    ARG_CHECK_CTX(ctx, true, "reloc_obs_get_filter");
    const ObstacleState &o = ctx->obs;
    if (bh) *bh = o.bh;
    if (bw) *bw = o.bw;
    if (lo) *lo = o.f_lo;
    if (hi) *hi = o.f_hi;
    if (min_count) *min_count = o.min_count;
    if (n_cov) *n_cov = o.n_cov;
    if (var_thresh) *var_thresh = o.var_thresh;
    if (min_solid) *min_solid = o.min_solid;
    if (fill) *fill = o.f_fill;
    return RELOC_OK;
}

RELOC_API int reloc_obs_filter_depth(reloc_ctx *ctx, const void *depth, int is_f32, int w, int h, float *filtered, uint8_t *mask)
{
    ARG_CHECK_CTX(ctx, depth && w > 0 && h > 0, "reloc_obs_filter_depth: an image of positive size");
    if (!ctx->obs.filter_on()) { reloc_set_error("reloc_obs_filter_depth: the traversability filter is off on this context (reloc_obs_set_filter)"); return RELOC_E_STATE; }
    HostStaging st{ctx};
    ObsFrame f;
    if (int rc = obs_source(st, depth, is_f32, w, h, false, "reloc_obs_filter_depth", f)) { st.finish(); return rc; }
    const ObsMask m = obs_mask(st, f, true);
    if (filtered) {
        float *d = st.slot<float>(6, (int64_t)w * h);
        st.launch(f.f32 ? k_obs_filtered<true> : k_obs_filtered<false>, dim3(grid_1d((int64_t)w * h, 2048)), dim3(256), f.src, m, d);
        st.download(filtered, d, (int64_t)w * h * 4);
    }
    if (mask && m.nby * m.nbx > 0) st.download(mask, m.mask, (int64_t)m.nby * m.nbx);
    return st.finish();
}

static int obs_profile(reloc_ctx *ctx, const void *depth, int is_f32, int w, int h, bool stereo, const ObsProfilePrm &p, float *profile,
                       int32_t *counts, const char *who)
{
    if (int rc = obs_profile_check(ctx, p, who)) return rc;
    HostStaging st{ctx};
    ObsFrame f;
    if (int rc = obs_source(st, depth, is_f32, w, h, stereo, who, f)) { st.finish(); return rc; }
    const int ncols = obs_profile_launch(st, f, p);
    if (profile) st.download(profile, ctx->obs.prof, (int64_t)ncols * 4);
    if (counts) st.download(counts, ctx->obs.cnt, (int64_t)ncols * 4);
    return stereo && !profile && !counts ? st.rc : st.finish();
}

RELOC_API int reloc_obs_profile_depth(reloc_ctx *ctx, const void *depth, int is_f32, int w, int h, int step, float lo, float hi, int q,
                                      int min_valid, float fill, int use_filter, float *profile, int32_t *counts)
{
    ARG_CHECK_CTX(ctx, depth && w > 0 && h > 0, "reloc_obs_profile_depth: an image of positive size");
    return obs_profile(ctx, depth, is_f32, w, h, false, ObsProfilePrm{step, lo, hi, q, min_valid, fill, use_filter}, profile, counts, "reloc_obs_profile_depth");
}

RELOC_API int reloc_obs_profile_stereo_dev(reloc_ctx *ctx, int step, float lo, float hi, int q, int min_valid, float fill, int use_filter,
                                           float *profile, int32_t *counts)
{
    ARG_CHECK_CTX(ctx, true, "reloc_obs_profile_stereo_dev");
    return obs_profile(ctx, nullptr, 0, 0, 0, true, ObsProfilePrm{step, lo, hi, q, min_valid, fill, use_filter}, profile, counts, "reloc_obs_profile_stereo_dev");
}

RELOC_API int reloc_obs_grid_configure(reloc_ctx *ctx, int cells, double res, float decay, float hit, float hit_nb, float obstacle_hits,
                                       int step, float lo, float hi, int q, int min_valid, int use_filter)
{
    ARG_CHECK_CTX(ctx, cells > 0 && occ_finite(res) && res > 0 && occ_finite(decay) && decay > 0 && occ_finite(hit) && hit > 0 && occ_finite(hit_nb) &&
                           hit_nb > 0 && occ_finite(obstacle_hits) && obstacle_hits > 0,
                  "reloc_obs_grid_configure: cells, res, decay, hit, hit_nb and obstacle_hits must be positive and finite");
    if (int rc = obs_profile_check(ctx, ObsProfilePrm{step, lo, hi, q, min_valid, 0.0f, use_filter}, "reloc_obs_grid_configure")) return rc;
    if (cells > RELOC_OBS_MAX_CELLS) {
        reloc_set_error("reloc_obs_grid_configure: %d cells per side exceed the capacity (%d)", cells, RELOC_OBS_MAX_CELLS);
        return RELOC_E_CAPACITY;
    }
    ObstacleState &o = ctx->obs;
    const int64_t n = (int64_t)cells * cells;
    if (int rc = o.grid_block.layout(ctx, [&](BlockCarver &c) {
            c(o.grid[0], n);
            c(o.grid[1], n);
            c(o.stats, 2);
            c(o.image, n);
        })) return rc;
    o.cells = 0;
    HIP_TRY(hipMemsetAsync(o.grid[0], 0, (size_t)n * 4, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    o.cells = cells; o.cur = 0; o.res = res; o.decay = decay; o.hit = hit; o.hit_nb = hit_nb; o.obstacle_hits = obstacle_hits;
    o.step = step; o.lo = lo; o.hi = hi; o.q = q; o.min_valid = min_valid; o.use_filter = use_filter;
    return RELOC_OK;
}

static int obs_need_grid(const reloc_ctx *ctx, const char *who)
{
    if (!ctx->obs.on()) reloc_set_error("%s: no obstacle grid on this context (reloc_obs_grid_configure)", who);
    return ctx->obs.on() ? RELOC_OK : RELOC_E_STATE;
}

// The directions of an enqueue-only update: through the context's pinned table, so that nothing of the caller's memory is in
// flight when the entry point returns; the table is free again once the copy out of it has run (dirs_read).
static int obs_dirs_enqueue(reloc_ctx *ctx, const double *dirs, int ncols, double *dev, const double2 **out)
{
    ObstacleState &o = ctx->obs;
    if (!dev) return RELOC_E_HIP;
    if (!o.dirs_host) {
        HIP_TRY(hipHostMalloc((void **)&o.dirs_host, sizeof(double) * 2 * RELOC_OBS_MAX_GRID_COLS, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&o.dirs_read, hipEventDisableTiming));
    } else HIP_TRY(hipEventSynchronize(o.dirs_read));
    memcpy(o.dirs_host, dirs, sizeof(double) * 2 * ncols);
    HIP_TRY(hipMemcpyAsync(dev, o.dirs_host, sizeof(double) * 2 * ncols, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(o.dirs_read, ctx->stream));
    *out = (const double2 *)dev;
    return RELOC_OK;
}

void obs_release(reloc_ctx *ctx)
{
    if (ctx->obs.dirs_read) (void)hipEventDestroy(ctx->obs.dirs_read);
    if (ctx->obs.dirs_host) (void)hipHostFree(ctx->obs.dirs_host);
}

// One update; have_depth: a host image or (stereo) the dense plane is projected along dirs.  wait: synchronises.
static int obs_grid_update(reloc_ctx *ctx, int sx, int sy, bool have_depth, const void *depth, int is_f32, int w, int h, bool stereo,
                           const double *dirs, int n_dirs, bool wait, const char *who)
{
    if (int rc = obs_need_grid(ctx, who)) return rc;
    ObstacleState &o = ctx->obs;
    const ObsProfilePrm p{o.step, o.lo, o.hi, o.q, o.min_valid, 0.0f, o.use_filter};
    if (have_depth)
        if (int rc = obs_profile_check(ctx, p, who)) return rc;      // the filter may have been switched off since
    HostStaging st{ctx};
    int ncols = 0;
    const double2 *ddirs = nullptr;
    if (have_depth) {
        ObsFrame f;
        if (int rc = obs_source(st, depth, is_f32, w, h, stereo, who, f)) { st.finish(); return rc; }
        ncols = (f.src.w + o.step - 1) / o.step;
        if (!dirs || n_dirs != ncols) {
            st.finish();
            reloc_set_error("bad argument: %s: %d directions for %d columns", who, n_dirs, ncols);
            return RELOC_E_ARG;
        }
        if (ncols > RELOC_OBS_MAX_GRID_COLS) {
            st.finish();
            reloc_set_error("%s: %d columns exceed the capacity (%d)", who, ncols, RELOC_OBS_MAX_GRID_COLS);
            return RELOC_E_CAPACITY;
        }
        for (int k = 0; k < 2 * ncols; ++k)
            if (!occ_finite(dirs[k])) { st.finish(); reloc_set_error("bad argument: %s: the directions must be finite", who); return RELOC_E_ARG; }
        obs_profile_launch(st, f, p);
        if (wait) ddirs = (const double2 *)st.upload_slot(6, dirs, (int64_t)2 * ncols);
        else st.run([&] { return obs_dirs_enqueue(ctx, dirs, ncols, st.slot<double>(6, (int64_t)2 * ncols), &ddirs); });
    }
    const int cells = o.cells;
    const int csx = sx > cells ? cells : sx < -cells ? -cells : sx, csy = sy > cells ? cells : sy < -cells ? -cells : sy;
    st.launch(k_obs_grid_update, dim3(grid_1d((int64_t)cells * cells, 256)), dim3(256), (const float *)o.grid[o.cur], o.grid[o.cur ^ 1], cells, csx, csy,
              o.decay, (const float *)o.prof, (const int32_t *)o.cnt, ddirs, ncols, o.min_valid, o.res, o.hit, o.hit_nb);
    const int rc = wait ? st.finish() : st.rc;
    if (!rc) o.cur ^= 1;
    return rc;
}

RELOC_API int reloc_obs_grid_update_depth(reloc_ctx *ctx, int sx, int sy, const void *depth, int is_f32, int w, int h, const double *dirs,
                                          int n_dirs)
{
    ARG_CHECK_CTX(ctx, !depth || (w > 0 && h > 0), "reloc_obs_grid_update_depth: an image of positive size, or none");
    return obs_grid_update(ctx, sx, sy, depth != nullptr, depth, is_f32, w, h, false, dirs, n_dirs, true, "reloc_obs_grid_update_depth");
}

RELOC_API int reloc_obs_grid_update_stereo_dev(reloc_ctx *ctx, int sx, int sy, const double *dirs, int n_dirs)
{
    ARG_CHECK_CTX(ctx, dirs && n_dirs > 0, "reloc_obs_grid_update_stereo_dev: the directions of the plane's columns");
    return obs_grid_update(ctx, sx, sy, true, nullptr, 0, 0, 0, true, dirs, n_dirs, false, "reloc_obs_grid_update_stereo_dev");
}

RELOC_API int reloc_obs_grid_profile(reloc_ctx *ctx, const double *dirs, int n, double max_range, double *out)
{
    ARG_CHECK_CTX(ctx, n >= 0 && ((dirs && out) || n == 0) && occ_finite(max_range), "reloc_obs_grid_profile: n >= 0 directions and their output, a finite range");
    if (int rc = obs_need_grid(ctx, "reloc_obs_grid_profile")) return rc;
    const ObstacleState &o = ctx->obs;
    for (int k = 0; k < 2 * n; ++k)
        if (!occ_finite(dirs[k])) { reloc_set_error("bad argument: reloc_obs_grid_profile: the directions must be finite"); return RELOC_E_ARG; }
    if (n > RELOC_OBS_MAX_SECTORS || max_range / o.res > (double)RELOC_OBS_MAX_STEPS) {
        reloc_set_error("reloc_obs_grid_profile: %d sectors or %g steps exceed the capacity (%d, %d)", n, max_range / o.res, RELOC_OBS_MAX_SECTORS, RELOC_OBS_MAX_STEPS);
        return RELOC_E_CAPACITY;
    }
    if (n == 0) return RELOC_OK;
    HostStaging st{ctx};
    const double2 *d = (const double2 *)st.upload_slot(6, dirs, (int64_t)2 * n);
    double *dout = st.slot<double>(7, n);
    st.launch(k_obs_rays, dim3((n + 63) / 64), dim3(64), (const float *)o.grid[o.cur], o.cells, d, n, o.res, max_range, o.obstacle_hits, dout);
    st.download(out, dout, (int64_t)n * 8);
    return st.finish();
}

RELOC_API int reloc_obs_grid_read(reloc_ctx *ctx, float *grid, uint8_t *image, int32_t *obstacle_cells, float *max_hits, int32_t *cells)
{
    ARG_CHECK_CTX(ctx, true, "reloc_obs_grid_read");
    if (int rc = obs_need_grid(ctx, "reloc_obs_grid_read")) return rc;
    const ObstacleState &o = ctx->obs;
    const int64_t n = (int64_t)o.cells * o.cells;
    if (cells) *cells = o.cells;
    HostStaging st{ctx};
    int32_t stats[2] = {0, 0};
    if (grid) st.download(grid, o.grid[o.cur], n * 4);
    if (image || obstacle_cells || max_hits) {
        st.launch(k_obs_readout, dim3(1), dim3(1024), (const float *)o.grid[o.cur], (int)n, o.obstacle_hits, o.image, o.stats);
        if (image) st.download(image, o.image, n);
        st.download(stats, o.stats, 8);
    }
    if (int rc = st.finish()) return rc;
    if (obstacle_cells) *obstacle_cells = stats[0];
    if (max_hits) memcpy(max_hits, &stats[1], 4);
    return RELOC_OK;
}

RELOC_API int reloc_morph_rect(reloc_ctx *ctx, const uint8_t *src, int w, int h, int stride, int kw, int kh, int dilate, int iterations,
                               uint8_t *dst)
{
    ARG_CHECK_CTX(ctx, src && dst && w > 0 && h > 0 && stride >= w && kw >= 1 && kh >= 1 && iterations >= 1 && (dilate == 0 || dilate == 1),
                  "reloc_morph_rect: images, positive sizes, stride >= w, kernel sides and iterations >= 1, dilate 0 or 1");
    if ((int64_t)w * h > (int64_t)ctx->max_w * ctx->max_h || kw > RELOC_MORPH_MAX_KERNEL || kh > RELOC_MORPH_MAX_KERNEL || iterations > RELOC_MORPH_MAX_ITERATIONS) {
        reloc_set_error("reloc_morph_rect: image %d x %d, kernel %d x %d or %d iterations exceed the capacity (ctx %d x %d, side %d, %d iterations)", w, h, kw, kh,
                        iterations, ctx->max_w, ctx->max_h, RELOC_MORPH_MAX_KERNEL, RELOC_MORPH_MAX_ITERATIONS);
        return RELOC_E_CAPACITY;
    }
    HostStaging st{ctx};
    const int64_t n = (int64_t)w * h;
    uint8_t *buf[2] = {st.slot<uint8_t>(5, n), st.slot<uint8_t>(6, n)};
    st.upload_rows(buf[0], src, w, h, stride);
    int cur = 0;
    const dim3 grid(grid_1d(n, 2048)), block(256);
    for (int it = 0; it < iterations; ++it) {
        if (kw > 1) {
            st.launch(dilate ? k_morph_pass<true, true> : k_morph_pass<false, true>, grid, block, (const uint8_t *)buf[cur], buf[cur ^ 1], w, h, kw, kw / 2);
            cur ^= 1;
        }
        if (kh > 1) {
            st.launch(dilate ? k_morph_pass<true, false> : k_morph_pass<false, false>, grid, block, (const uint8_t *)buf[cur], buf[cur ^ 1], w, h, kh, kh / 2);
            cur ^= 1;
        }
    }
    st.download(dst, buf[cur], n);
    return st.finish();
}
