// reloc_occupancy.hip -- teach-time occupancy map (include/reloc_spec.h "OCCUPANCY"; DESIGN.md "Occupancy map").
// A frame is two launches on the context's stream:
//   k_occ_integrate  one workgroup of 1024: depth pixel (depth_grid_point) or cloud row -> sensor point -> map point -> filters
//                    -> ordered rank (block_rank, as k_depth_points; the cloud is never written), rays queued in LDS and
//                    walked one per lane, 1024 at a time.  The cells of a OCC_WIN x OCC_WIN window around the start cell are
//                    summed in LDS and applied to the grid once; the start cell itself, which every ray crosses, is summed in
//                    registers and added once per wave.  Cells beyond the window take global int32 atomics into `acc`.
//   k_occ_apply      v = clamp(v + acc) and acc = 0 over the box that the frame's far rays span (nothing when there are none).
// Integer sums only: the grid is the same whatever order the adds arrive in.
#include "reloc_teach.h"

// Developer switch for A/B builds (build.build_variant, tools/exp_occupancy.py): 2 = the shipped form; 1 = only the start cell is
// summed on chip, every other cell takes a global atomic; 0 = every update is a global atomic.  The grid is the same in all.
#ifndef RELOC_OCC_FORM
#define RELOC_OCC_FORM 2
#endif
constexpr int OCC_WIN = 112;          // side of the on-chip window, cells; the start cell is its cell (OCC_WIN / 2, OCC_WIN / 2)
constexpr int OCC_QUEUE = 2048;       // rays waiting in LDS: drained when more than 1024 wait, so a chunk's 1024 always fit
constexpr int OCC_MAX_SIDE = 32768;   // a queued end cell is row << 16 | col

struct OccGeom { double ox, oy, res, z_lo, z_hi; int W, H, sub; };
// frame record on the device: [0] rays of the frame, [1..4] box of the far rays (row lo, row hi, col lo, col hi; hi < lo: none)
constexpr int OCC_FRAME_WORDS = 8;

template <int SRC>
__global__ __launch_bounds__(1024) void k_occ_integrate(OccSrc src, OccT T, OccGeom g, int8_t *__restrict__ units,
                                                        int32_t *__restrict__ acc, int64_t *__restrict__ counters,
                                                        int32_t *__restrict__ frame)
{
    __shared__ int s_win[OCC_WIN * OCC_WIN];
    __shared__ unsigned s_queue[OCC_QUEUE];
    __shared__ int s_wsum[16];
    __shared__ int s_fin, s_qn;
    __shared__ int s_box[4];                      // row lo, row hi, col lo, col hi of the end cells beyond the window
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < OCC_WIN * OCC_WIN; i += 1024) s_win[i] = 0;
    if (tid == 0) { s_fin = 0; s_qn = 0; s_box[0] = g.H; s_box[1] = -1; s_box[2] = g.W; s_box[3] = -1; }
    int r0, c0;
    const bool start_in = occ_cell(T.v[3], g.ox, g.res, g.W, c0) & occ_cell(T.v[7], g.oy, g.res, g.H, r0);
    const int wr0 = r0 - OCC_WIN / 2, wc0 = c0 - OCC_WIN / 2;
    const int n = occ_src_count<SRC>(src);
    int at_start = 0;                             // this lane's share of the start cell's sum
    int n_fin = 0, n_keep = 0;                    // this lane's finite points; the workgroup's kept points so far
    __syncthreads();

    // the rays waiting in the queue, one per lane
    auto drain = [&]() {
        const int qn = s_qn;
        for (int q = tid; q < qn; q += 1024) {
            const unsigned e = s_queue[q];
            const int r1 = (int)(e >> 16), c1 = (int)(e & 0xFFFFu);
            const int dr = abs(r1 - r0), dc = abs(c1 - c0);
            const int sr = r0 < r1 ? 1 : -1, sc = c0 < c1 ? 1 : -1;
            int err = dr - dc, r = r0, c = c0;
            for (int it = 0; it <= dr + dc; ++it) {               // D:172-195; a walk takes max(dr, dc) steps
                const bool end = r == r1 && c == c1;
                const int d = end ? RELOC_OCC_L_OCC : RELOC_OCC_L_FREE;
                const int wr = r - wr0, wc = c - wc0;
                if (it == 0 && RELOC_OCC_FORM >= 1) at_start += d;
                else if (RELOC_OCC_FORM >= 2 && (unsigned)wr < (unsigned)OCC_WIN && (unsigned)wc < (unsigned)OCC_WIN) atomicAdd(&s_win[wr * OCC_WIN + wc], d);
                else if ((unsigned)r < (unsigned)g.H && (unsigned)c < (unsigned)g.W) atomicAdd(&acc[r * g.W + c], d);
                if (end) break;
                const int e2 = 2 * err;
                if (e2 > -dc) { err -= dc; r += sr; }
                if (e2 < dr) { err += dr; c += sc; }
            }
        }
        __syncthreads();
        if (tid == 0) s_qn = 0;
        __syncthreads();
    };

    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        bool fin = false, keep = false;
        double mx = 0, my = 0;
        if (i < n) {
            float p[3];
            fin = occ_src_point<SRC>(src, i, p);
            if (fin) {
                mx = occ_map_coord(T, 0, p);
                my = occ_map_coord(T, 1, p);
                const double mz = occ_map_coord(T, 2, p);
                keep = mz > g.z_lo && mz < g.z_hi;
            }
        }
        n_fin += fin;
        int total;
        const int rank = block_rank(keep, s_wsum, n_keep, total);      // among the kept points, which is what sub counts
        n_keep += total;
        if (keep && start_in) {
            int r1, c1;
            if (rank % g.sub == 0 && (occ_cell(mx, g.ox, g.res, g.W, c1) & occ_cell(my, g.oy, g.res, g.H, r1))) {
                s_queue[atomicAdd(&s_qn, 1)] = (unsigned)r1 << 16 | (unsigned)c1;
                if (RELOC_OCC_FORM < 2 || (unsigned)(r1 - wr0) >= (unsigned)OCC_WIN || (unsigned)(c1 - wc0) >= (unsigned)OCC_WIN) {
                    atomicMin(&s_box[0], r1); atomicMax(&s_box[1], r1); atomicMin(&s_box[2], c1); atomicMax(&s_box[3], c1);
                }
            }
        }
        __syncthreads();
        if (s_qn > 1024) drain();
    }
    drain();

    // the start cell and the finite points: one add per wave
    const int wave_start = wave_sum_i32(at_start), wave_fin = wave_sum_i32(n_fin);
    if (lane == 0 && wave_start != 0) atomicAdd(&s_win[(OCC_WIN / 2) * OCC_WIN + OCC_WIN / 2], wave_start);
    if (lane == 0 && wave_fin != 0) atomicAdd(&s_fin, wave_fin);
    __syncthreads();
    // the window: one clamped update per cell, straight into the grid (no far add ever lands on a window cell)
    for (int i = tid; i < OCC_WIN * OCC_WIN; i += 1024) {
        const int d = s_win[i];
        const int r = wr0 + i / OCC_WIN, c = wc0 + i % OCC_WIN;
        if (d != 0 && (unsigned)r < (unsigned)g.H && (unsigned)c < (unsigned)g.W) {
            const int v = (int)units[r * g.W + c] + d;
            units[r * g.W + c] = (int8_t)min(max(v, RELOC_OCC_L_MIN), RELOC_OCC_L_MAX);
        }
    }
    if (tid == 0) {                               // (h)
        int rays = 0;
        if (s_fin == 0) counters[2] += 1;
        else if (n_keep > 0 && start_in) {
            rays = (n_keep + g.sub - 1) / g.sub;
            counters[0] += 1;
            counters[1] += rays;
        }
        frame[0] = rays;
        const bool far = s_box[1] >= 0;            // the far cells of a ray lie in the box its two ends span
        frame[1] = far ? min(s_box[0], r0) : 1; frame[2] = far ? max(s_box[1], r0) : 0;
        frame[3] = far ? min(s_box[2], c0) : 1; frame[4] = far ? max(s_box[3], c0) : 0;
    }
}

__global__ __launch_bounds__(256) void k_occ_apply(int8_t *__restrict__ units, int32_t *__restrict__ acc, const int32_t *__restrict__ frame,
                                                   int W, int H)
{
    const int r_lo = max(frame[1], 0), r_hi = min(frame[2], H - 1), c_lo = max(frame[3], 0), c_hi = min(frame[4], W - 1);
    if (r_hi < r_lo || c_hi < c_lo) return;
    const int bw = c_hi - c_lo + 1, n = bw * (r_hi - r_lo + 1);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int idx = (r_lo + i / bw) * W + c_lo + i % bw;
        const int d = acc[idx];
        if (d != 0) {
            units[idx] = (int8_t)min(max((int)units[idx] + d, RELOC_OCC_L_MIN), RELOC_OCC_L_MAX);
            acc[idx] = 0;
        }
    }
}

// (f): the .pgm's plane, rows flipped
__global__ __launch_bounds__(256) void k_occ_classify(const int8_t *__restrict__ units, uint8_t *__restrict__ pgm, int W, int H)
{
    const int n = W * H;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int v = units[i], r = i / W, c = i % W;
        pgm[(H - 1 - r) * W + c] = v >= RELOC_OCC_UNITS_OCC ? RELOC_OCC_PGM_OCC : v <= RELOC_OCC_UNITS_FREE ? RELOC_OCC_PGM_FREE : RELOC_OCC_PGM_UNKNOWN;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
RELOC_API int reloc_occ_configure(reloc_ctx *ctx, double origin_x, double origin_y, double res, int w_cells, int h_cells, double z_lo,
                                  double z_hi, int subsample)
{
    ARG_CHECK_CTX(ctx, w_cells > 0 && h_cells > 0 && subsample > 0 && occ_finite(origin_x) && occ_finite(origin_y) && occ_finite(res) &&
                           res > 0 && occ_finite(z_lo) && occ_finite(z_hi),
                  "reloc_occ_configure: sizes, res and subsample must be positive, everything finite");
    if (w_cells > OCC_MAX_SIDE || h_cells > OCC_MAX_SIDE || (int64_t)w_cells * h_cells > RELOC_OCC_MAX_CELLS) {
        reloc_set_error("occupancy grid %d x %d exceeds the capacity (%d cells, %d per side)", w_cells, h_cells, RELOC_OCC_MAX_CELLS, OCC_MAX_SIDE);
        return RELOC_E_CAPACITY;
    }
    OccState &o = ctx->occ;
    const int64_t cells = (int64_t)w_cells * h_cells;
    if (int rc = o.block.layout(ctx, [&](BlockCarver &c) {
            c(o.acc, cells);
            c(o.counters, 3);
            c(o.frame, OCC_FRAME_WORDS);
            c(o.units, cells);
            c(o.pgm, cells);
        })) return rc;
    o.w = w_cells; o.h = h_cells; o.sub = subsample;
    o.ox = origin_x; o.oy = origin_y; o.res = res; o.z_lo = z_lo; o.z_hi = z_hi;
    HIP_TRY(hipMemsetAsync(o.block.p, 0, (size_t)(o.pgm + cells - o.block.p), ctx->stream));      // what this geometry takes of the block
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RELOC_OK;
}

static int occ_check(reloc_ctx *ctx, const double *T12, const char *who)
{
    if (int rc = occ_need_map(ctx, who)) return rc;
    return frame_transform_check(T12, who);
}

// A frame: the two launches on the context's stream, then the frame's rays into *out_rays (may be NULL); !wait: enqueues only.
static int occ_frame(reloc_ctx *ctx, HostStaging &st, const FrameSrc &f, const double *T12, int32_t *out_rays, bool wait)
{
    const OccState &o = ctx->occ;
    OccT T;
    memcpy(T.v, T12, sizeof(T.v));
    const OccGeom g{o.ox, o.oy, o.res, o.z_lo, o.z_hi, o.w, o.h, o.sub};
    st.launch(FRAME_KERNEL(k_occ_integrate, f.kind), dim3(1), dim3(1024), f.src, T, g, o.units, o.acc, o.counters, o.frame);
    st.launch(k_occ_apply, dim3(64), dim3(256), o.units, o.acc, (const int32_t *)o.frame, o.w, o.h);
    if (!wait) return st.rc;
    const int32_t rays = st.count(o.frame);
    if (int rc = st.finish()) return rc;
    if (out_rays) *out_rays = rays;
    return RELOC_OK;
}

RELOC_API int reloc_occ_integrate_points(reloc_ctx *ctx, const float *pts, int n, const double T12[12], int32_t *out_rays)
{
    ARG_CHECK_CTX(ctx, n >= 0 && (pts || n == 0) && T12, "reloc_occ_integrate_points");
    if (int rc = occ_check(ctx, T12, "reloc_occ_integrate_points")) return rc;
    HostStaging st{ctx};
    return occ_frame(ctx, st, frame_from_cloud(st, pts, n), T12, out_rays, true);
}

RELOC_API int reloc_occ_integrate_depth(reloc_ctx *ctx, const void *depth, int is_f32, int w, int h, int step, const double K4[4],
                                        float zmin, float zmax, const double T12[12], int32_t *out_rays)
{
    ARG_CHECK_CTX(ctx, depth && w > 0 && h > 0 && step > 0 && K4 && T12, "reloc_occ_integrate_depth");
    if (int rc = occ_check(ctx, T12, "reloc_occ_integrate_depth")) return rc;
    HostStaging st{ctx};
    return occ_frame(ctx, st, frame_from_depth(st, depth, is_f32, w, h, step, K4, zmin, zmax), T12, out_rays, true);
}

// The plane of the last dense stereo pass where it lies.  out_rays == NULL: enqueues only, the host never waits.
RELOC_API int reloc_occ_integrate_stereo_dev(reloc_ctx *ctx, int step, float zmin, float zmax, const double T12[12], int32_t *out_rays)
{
    ARG_CHECK_CTX(ctx, step > 0 && T12, "reloc_occ_integrate_stereo_dev");
    if (int rc = occ_check(ctx, T12, "reloc_occ_integrate_stereo_dev")) return rc;
    HostStaging st{ctx};
    return occ_frame(ctx, st, frame_from_stereo(st, step, zmin, zmax), T12, out_rays, out_rays != nullptr);
}

RELOC_API int reloc_occ_read(reloc_ctx *ctx, int8_t *units, uint8_t *pgm, int64_t counters[3])
{
    ARG_CHECK_CTX(ctx, true, "reloc_occ_read");
    if (int rc = occ_need_map(ctx, "reloc_occ_read")) return rc;
    const OccState &o = ctx->occ;
    const int64_t cells = (int64_t)o.w * o.h;
    HostStaging st{ctx};
    if (units) st.download(units, o.units, cells);
    if (pgm) {
        st.launch(k_occ_classify, dim3(grid_1d(cells, 1024)), dim3(256), (const int8_t *)o.units, o.pgm, o.w, o.h);
        st.download(pgm, o.pgm, cells);
    }
    if (counters) st.download(counters, o.counters, 3 * 8);
    return st.finish();
}
