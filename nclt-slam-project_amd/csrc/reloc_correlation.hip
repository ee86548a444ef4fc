// reloc_correlation.hip -- depth-correlation anchor (include/reloc_spec.h "CORRELATION"; DESIGN.md "Depth-correlation anchor").
// Everything is bit arithmetic on one bit per cell, 32 cells per word, bit b of word k = column 32 k + b.
// Once per map:
//   k_corr_pack      the occupied plane (uint8, or the occupancy map's int8 units) -> packed rows of MP = ceil(W / 32) words,
//                    the bits beyond column W - 1 clear
//   k_corr_dilate    one iteration of the 4-connected cross, n launches ping-pong between the two halves of the map's block
// A tick is three launches on the context's stream:
//   k_corr_scan      one workgroup of 1024: source row -> sensor point -> map point -> filters -> cell, as k_occ_integrate reads
//                    and maps it; the three populations are counted, the cells set bits in an LDS bitmap of the S x S window
//                    around the base cell (distinct cells for free, n_cells its popcount); its non-zero words go to HBM as a
//                    list of (row << 5 | word index, bits)
//   k_corr_correlate one wave per offset (i, j), lanes over the list: popcount(scan word & the map's 32 cells at the shifted
//                    position, funnel-shifted to the column phase); words beyond the map read as 0
//   k_corr_pick      best in C's order (max over hits << 32 | ~order), second, into the record
// Integer sums only: the surface is the same whatever order they arrive in.
#include "reloc_teach.h"

// (A list of cells with one bit test per offset and cell was measured against the list of words: profiles/README.md, "Dropped experiments" #11.)
constexpr int CORR_WIN_WORDS = (RELOC_CORR_MAX_WINDOW + 31) / 32;                  // words per window row at the largest window
constexpr int CORR_REC_DEV = 16;                                                    // the record on the device: [8] = cells lost, [9] = listed words
// the scan's list: a non-zero word of the window as two words, (row << 5 | word index, bits)
constexpr size_t CORR_LIST_WORDS = (size_t)2 * RELOC_CORR_MAX_WINDOW * CORR_WIN_WORDS;
constexpr int CORR_BASE_CLAMP = 1 << 29;                                            // base cell, so that no index sum wraps

struct CorrGeom {
    double ox, oy, res, z_lo, z_hi, vx, vy, rr;
    int W, H, wr0, wc0, S, PW, min_points;
};

template <int FROM_UNITS>
__global__ __launch_bounds__(256) void k_corr_pack(const void *__restrict__ plane, uint32_t *__restrict__ map, int W, int H, int MP)
{
    const int n = H * MP;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += gridDim.x * blockDim.x) {
        const int r = idx / MP, k = idx % MP;
        uint32_t word = 0;
        for (int b = 0; b < 32; ++b) {
            const int c = 32 * k + b;
            if (c < W) {
                const size_t at = (size_t)r * W + c;
                const bool occ = FROM_UNITS ? reinterpret_cast<const int8_t *>(plane)[at] >= RELOC_OCC_UNITS_OCC
                                            : reinterpret_cast<const uint8_t *>(plane)[at] != 0;
                word |= (uint32_t)occ << b;
            }
        }
        map[idx] = word;
    }
}

// (a): the cross, carries across words, nothing beyond the border
__global__ __launch_bounds__(256) void k_corr_dilate(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, int W, int H, int MP)
{
    const int n = H * MP;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += gridDim.x * blockDim.x) {
        const int r = idx / MP, k = idx % MP;
        const uint32_t w = in[idx];
        const uint32_t left = k > 0 ? in[idx - 1] : 0u, right = k + 1 < MP ? in[idx + 1] : 0u;
        const uint32_t up = r > 0 ? in[idx - MP] : 0u, down = r + 1 < H ? in[idx + MP] : 0u;
        uint32_t v = w | (w << 1) | (left >> 31) | (w >> 1) | (right << 31) | up | down;
        if (k == MP - 1 && (W & 31)) v &= (1u << (W & 31)) - 1u;
        out[idx] = v;
    }
}

__global__ __launch_bounds__(256) void k_corr_unpack(const uint32_t *__restrict__ map, uint8_t *__restrict__ plane, int W, int H, int MP)
{
    const int n = W * H;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int r = i / W, c = i % W;
        plane[i] = (uint8_t)(map[r * MP + (c >> 5)] >> (c & 31) & 1u);
    }
}

template <int SRC>
__global__ __launch_bounds__(1024) void k_corr_scan(OccSrc src, OccT T, CorrGeom g, uint32_t *__restrict__ list, int32_t *__restrict__ rec)
{
    extern __shared__ uint32_t s_bits[];          // S rows of PW words
    __shared__ int s_cnt[6];                      // finite, kept, in the map, distinct cells, lost, listed
    const int tid = threadIdx.x, lane = tid & 63;
    const int nw = g.S * g.PW;
    for (int i = tid; i < nw; i += 1024) s_bits[i] = 0u;
    if (tid < 6) s_cnt[tid] = 0;
    __syncthreads();
    const int n = occ_src_count<SRC>(src);
    int n_fin = 0, n_keep = 0, n_in = 0, n_lost = 0;
    for (int i = tid; i < n; i += 1024) {
        float p[3];
        if (!occ_src_point<SRC>(src, i, p)) continue;                                          // (b)
        ++n_fin;
        const double mx = occ_map_coord(T, 0, p), my = occ_map_coord(T, 1, p), mz = occ_map_coord(T, 2, p);      // (c)
        const double dx = __dsub_rn(mx, g.vx), dy = __dsub_rn(my, g.vy);
        if (!(mz > g.z_lo && mz < g.z_hi && __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) < g.rr)) continue;      // (d)
        ++n_keep;
        int r, c;
        if (!(occ_cell(mx, g.ox, g.res, g.W, c) & occ_cell(my, g.oy, g.res, g.H, r))) continue;                   // (e)
        ++n_in;
        const int wr = r - g.wr0, wc = c - g.wc0;
        if ((unsigned)wr < (unsigned)g.S && (unsigned)wc < (unsigned)g.S) atomicOr(&s_bits[wr * g.PW + (wc >> 5)], 1u << (wc & 31));
        else ++n_lost;                            // the window holds every cell within max_range of the base cell: never taken
    }
    const int w_fin = wave_sum_i32(n_fin), w_keep = wave_sum_i32(n_keep), w_in = wave_sum_i32(n_in), w_lost = wave_sum_i32(n_lost);
    if (lane == 0) {
        if (w_fin) atomicAdd(&s_cnt[0], w_fin);
        if (w_keep) atomicAdd(&s_cnt[1], w_keep);
        if (w_in) atomicAdd(&s_cnt[2], w_in);
        if (w_lost) atomicAdd(&s_cnt[4], w_lost);
    }
    __syncthreads();
    int n_cells = 0;                              // (f); the list: one slot range per wave and turn, in no particular order
    for (int i0 = 0; i0 < nw; i0 += 1024) {
        const int i = i0 + tid;
        const uint32_t w = i < nw ? s_bits[i] : 0u;
        n_cells += __popc(w);
        const int take = w != 0u;
        const unsigned long long any = __ballot(take != 0);
        if (any == 0ull) continue;
        int mine = take;                          // inclusive scan: the entries of this lane and of those below it
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(mine, d);
            if (lane >= d) mine += v;
        }
        int base = 0;
        if (lane == 63) base = atomicAdd(&s_cnt[5], mine);
        const int at = __shfl(base, 63) + mine - take;
        if (w) {
            list[2 * at] = (uint32_t)(i / g.PW) << 5 | (uint32_t)(i % g.PW);
            list[2 * at + 1] = w;
        }
    }
    n_cells = wave_sum_i32(n_cells);
    if (lane == 0 && n_cells) atomicAdd(&s_cnt[3], n_cells);
    __syncthreads();
    if (tid == 0) {
        const int status = s_cnt[0] == 0 ? RELOC_CORR_NO_DEPTH_POINTS : s_cnt[1] < g.min_points ? RELOC_CORR_TOO_FEW_POINTS
                           : s_cnt[2] < g.min_points ? RELOC_CORR_OUT_OF_BOUNDS : RELOC_CORR_OK;
        rec[0] = status; rec[1] = s_cnt[1]; rec[2] = s_cnt[2];
        rec[3] = status == RELOC_CORR_OK ? s_cnt[3] : 0;
        rec[4] = rec[5] = rec[6] = rec[7] = 0;
        rec[8] = s_cnt[4]; rec[9] = s_cnt[5];
    }
}

// the map's 32 cells from column c on in row r (any c, any r): cells outside the map are 0
__device__ __forceinline__ uint32_t corr_map_bits(const uint32_t *__restrict__ map, int H, int MP, int r, int c)
{
    if ((unsigned)r >= (unsigned)H) return 0u;
    const int q = c >> 5;
    const uint32_t lo = (unsigned)q < (unsigned)MP ? map[r * MP + q] : 0u;
    const uint32_t hi = (unsigned)(q + 1) < (unsigned)MP ? map[r * MP + q + 1] : 0u;
    return __funnelshift_r(lo, hi, c & 31);
}

// (g): blockIdx.x = i, a wave per j; surface[i * n_side + j]
__global__ __launch_bounds__(256) void k_corr_correlate(const uint32_t *__restrict__ list, CorrGeom g, const uint32_t *__restrict__ map, int MP,
                                                        const int32_t *__restrict__ table, int n_side, const int32_t *__restrict__ rec,
                                                        int32_t *__restrict__ surface)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x, j = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (j >= n_side) return;
    int sum = 0;
    if (rec[0] == RELOC_CORR_OK) {
        const int dc = table[i], dr = table[j];
        const int n = rec[9];
        const uint2 *words = reinterpret_cast<const uint2 *>(list);
        for (int t = lane; t < n; t += 64) {
            const uint2 e = words[t];
            sum += __popc(e.y & corr_map_bits(map, g.H, MP, g.wr0 + (int)(e.x >> 5) + dr, g.wc0 + 32 * (int)(e.x & 31u) + dc));
        }
    }
    sum = wave_sum_i32(sum);
    if (lane == 0) surface[i * n_side + j] = sum;
}

// (h)
__global__ __launch_bounds__(1024) void k_corr_pick(const int32_t *__restrict__ surface, int n_side, int32_t *__restrict__ rec)
{
    __shared__ unsigned long long s_key;
    __shared__ int s_same, s_other;
    if (rec[0] != RELOC_CORR_OK) return;
    const int tid = threadIdx.x, lane = tid & 63, n2 = n_side * n_side;
    if (tid == 0) { s_key = 0ull; s_same = 0; s_other = 0; }
    __syncthreads();
    unsigned long long key = 0ull;                // the most hits, then the earliest in i-major order; 0: no offset has a hit
    for (int t = tid; t < n2; t += 1024) {
        const int h = surface[t];
        if (h > 0) key = max(key, (unsigned long long)h << 32 | (0xFFFFFFFFu - (unsigned)t));
    }
    for (int d = 32; d > 0; d >>= 1) key = max(key, (unsigned long long)__shfl_xor((long long)key, d));
    if (lane == 0 && key) atomicMax(&s_key, key);
    __syncthreads();
    const unsigned long long best = s_key;
    const int best_hits = (int)(best >> 32);
    int same = 0, other = 0;
    for (int t = tid; t < n2; t += 1024) {
        const int h = surface[t];
        same += h == best_hits;
        if (h != best_hits) other = max(other, h);
    }
    same = wave_sum_i32(same);
    for (int d = 32; d > 0; d >>= 1) other = max(other, __shfl_xor(other, d));
    if (lane == 0) { atomicAdd(&s_same, same); atomicMax(&s_other, other); }
    __syncthreads();
    if (tid == 0) {
        const int ns = n_side / 2, at = best ? (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)) : ns * n_side + ns;
        rec[4] = at / n_side - ns; rec[5] = at % n_side - ns; rec[6] = best_hits;
        rec[7] = n2 < 2 ? 0 : s_same >= 2 ? best_hits : s_other;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// half the window's side for a range and a cell size; RELOC_E_CAPACITY beyond RELOC_CORR_MAX_WINDOW
static int corr_window(double max_range, double res, int *half)
{
    const double cells = ceil(max_range / res);
    if (!(cells <= (double)((RELOC_CORR_MAX_WINDOW - 1) / 2 - 2))) {
        reloc_set_error("correlation window: max_range %g m at %g m per cell exceeds the capacity (%d cells per side)", max_range, res,
                        RELOC_CORR_MAX_WINDOW);
        return RELOC_E_CAPACITY;
    }
    *half = (int)cells + 2;
    return RELOC_OK;
}

// the checks of a new map, then its block: two packed planes of h rows of ceil(w / 32) words
static int corr_map_begin(reloc_ctx *ctx, int w, int h, double ox, double oy, double res, int dilate, const char *who)
{
    if (w > RELOC_CORR_MAX_SIDE || h > RELOC_CORR_MAX_SIDE || (int64_t)w * h > RELOC_CORR_MAX_CELLS) {
        reloc_set_error("%s: map %d x %d exceeds the capacity (%d cells, %d per side)", who, w, h, RELOC_CORR_MAX_CELLS, RELOC_CORR_MAX_SIDE);
        return RELOC_E_CAPACITY;
    }
    if (dilate > RELOC_CORR_MAX_DILATE) { reloc_set_error("%s: %d dilations exceed the capacity (%d)", who, dilate, RELOC_CORR_MAX_DILATE); return RELOC_E_CAPACITY; }
    CorrState &s = ctx->corr;
    int half = 0;
    if (s.configured())
        if (int rc = corr_window(s.max_range, res, &half)) return rc;
    const int mp = (w + 31) / 32;
    if (int rc = s.map_block.layout(ctx, [&](BlockCarver &c) { for (uint32_t *&plane : s.plane) c(plane, (int64_t)mp * h); })) return rc;
    s.w = w; s.h = h; s.mp = mp; s.ox = ox; s.oy = oy; s.res = res;
    if (s.configured()) s.half = half;
    return RELOC_OK;
}

// `plane` (device memory: h x w uint8, or the occupancy map's int8 units) as h packed rows of mp = ceil(w / 32) words at `bits`
void corr_pack_plane(HostStaging &st, const void *plane, bool from_units, uint32_t *bits, int w, int h, int mp)
{
    st.launch(from_units ? k_corr_pack<1> : k_corr_pack<0>, dim3(grid_1d((int64_t)mp * h, 1024)), dim3(256), plane, bits, w, h, mp);
}

// packs `plane` (device memory) into the map and dilates it; a failure leaves no map
static int corr_map_build(reloc_ctx *ctx, HostStaging &st, const void *plane, bool from_units, int dilate)
{
    CorrState &s = ctx->corr;
    corr_pack_plane(st, plane, from_units, s.plane[0], s.w, s.h, s.mp);
    for (int it = 0; it < dilate; ++it)
        st.launch(k_corr_dilate, dim3(grid_1d((int64_t)s.mp * s.h, 1024)), dim3(256), (const uint32_t *)s.plane[it & 1], s.plane[~it & 1], s.w, s.h, s.mp);
    s.map = s.plane[dilate & 1];
    const int rc = st.finish();
    if (rc) s.w = s.h = 0;
    return rc;
}

RELOC_API int reloc_corr_set_map(reloc_ctx *ctx, const uint8_t *occupied, int w, int h, double origin_x, double origin_y, double res, int dilate)
{
    ARG_CHECK_CTX(ctx, occupied && w > 0 && h > 0 && dilate >= 0 && occ_finite(origin_x) && occ_finite(origin_y) && occ_finite(res) && res > 0,
                  "reloc_corr_set_map: a plane, positive sizes and res, dilate >= 0, everything finite");
    if (int rc = corr_map_begin(ctx, w, h, origin_x, origin_y, res, dilate, "reloc_corr_set_map")) return rc;
    HostStaging st{ctx};
    return corr_map_build(ctx, st, st.upload_slot(6, occupied, (int64_t)w * h), false, dilate);
}

RELOC_API int reloc_corr_set_map_from_occ(reloc_ctx *ctx, int dilate)
{
    ARG_CHECK_CTX(ctx, dilate >= 0, "reloc_corr_set_map_from_occ: dilate >= 0");
    if (int rc = occ_need_map(ctx, "reloc_corr_set_map_from_occ")) return rc;
    const OccState &o = ctx->occ;
    if (int rc = corr_map_begin(ctx, o.w, o.h, o.ox, o.oy, o.res, dilate, "reloc_corr_set_map_from_occ")) return rc;
    HostStaging st{ctx};
    return corr_map_build(ctx, st, o.units, true, dilate);
}

static int corr_need_map(const reloc_ctx *ctx, const char *who) { return need_map(ctx->corr.on(), who, "correlation", "reloc_corr_set_map"); }


RELOC_API int reloc_corr_configure(reloc_ctx *ctx, const int32_t *cell_offsets, int n_side, double z_lo, double z_hi, double max_range, int min_points)
{
    ARG_CHECK_CTX(ctx, cell_offsets && n_side > 0 && (n_side & 1) && min_points >= 0 && occ_finite(z_lo) && occ_finite(z_hi) && occ_finite(max_range) &&
                           max_range > 0,
                  "reloc_corr_configure: an odd number of offsets, min_points >= 0, max_range > 0, everything finite");
    if (int rc = corr_need_map(ctx, "reloc_corr_configure")) return rc;
    if (n_side > RELOC_CORR_MAX_TABLE) { reloc_set_error("reloc_corr_configure: %d offsets exceed the capacity (%d)", n_side, RELOC_CORR_MAX_TABLE); return RELOC_E_CAPACITY; }
    for (int k = 0; k < n_side; ++k)
        if (cell_offsets[k] > RELOC_CORR_MAX_OFFSET || cell_offsets[k] < -RELOC_CORR_MAX_OFFSET) {
            reloc_set_error("reloc_corr_configure: offset %d of %d cells exceeds the capacity (%d)", k, cell_offsets[k], RELOC_CORR_MAX_OFFSET);
            return RELOC_E_CAPACITY;
        }
    CorrState &s = ctx->corr;
    int half = 0;
    if (int rc = corr_window(max_range, s.res, &half)) return rc;
    static_assert(RELOC_CORR_MAX_TABLE <= 256, "the table's room in the search's block");
    if (int rc = s.cfg_block.layout(ctx, [&](BlockCarver &c) {      // sized for the limits: taken once
            c.aligned<8>(s.list, CORR_LIST_WORDS);      // k_corr_correlate reads uint2
            c(s.surface, RELOC_CORR_MAX_TABLE * RELOC_CORR_MAX_TABLE);
            c(s.table, 256);
            c(s.record, CORR_REC_DEV);
        })) return rc;
    HostStaging st{ctx};
    st.upload(s.table, cell_offsets, (int64_t)n_side * 4);
    if (int rc = st.finish()) { s.n_side = 0; return rc; }
    s.n_side = n_side; s.z_lo = z_lo; s.z_hi = z_hi; s.max_range = max_range; s.min_points = min_points; s.half = half;
    return RELOC_OK;
}

static int corr_check(reloc_ctx *ctx, const double *T12, double vio_x, double vio_y, const char *who)
{
    if (int rc = corr_need_map(ctx, who)) return rc;
    if (!ctx->corr.configured()) { reloc_set_error("%s: the correlation search is not configured (reloc_corr_configure)", who); return RELOC_E_STATE; }
    if (int rc = frame_transform_check(T12, who)) return rc;
    if (!occ_finite(vio_x) || !occ_finite(vio_y)) { reloc_set_error("bad argument: %s: the base position must be finite", who); return RELOC_E_ARG; }
    return RELOC_OK;
}

static inline int corr_base_cell(double v, double origin, double res)
{
    const double q = floor((v - origin) / res);
    return q < -(double)CORR_BASE_CLAMP ? -CORR_BASE_CLAMP : q > (double)CORR_BASE_CLAMP ? CORR_BASE_CLAMP : (int)q;
}

// A tick: the three launches on the context's stream, then the record and the surface (may be NULL) to the host
static int corr_tick(reloc_ctx *ctx, HostStaging &st, const FrameSrc &f, const double *T12, double vio_x, double vio_y, int32_t *record,
                     int32_t *surface)
{
    const CorrState &s = ctx->corr;
    OccT T;
    memcpy(T.v, T12, sizeof(T.v));
    const int S = 2 * s.half + 1, PW = (S + 31) / 32;
    const CorrGeom g{s.ox, s.oy, s.res, s.z_lo, s.z_hi, vio_x, vio_y, s.max_range * s.max_range, s.w, s.h,
                     corr_base_cell(vio_y, s.oy, s.res) - s.half, corr_base_cell(vio_x, s.ox, s.res) - s.half, S, PW, s.min_points};
    const size_t lds = (size_t)S * PW * 4;
    st.run([&] {
        hipLaunchKernelGGL(FRAME_KERNEL(k_corr_scan, f.kind), dim3(1), dim3(1024), lds, ctx->stream, f.src, T, g, s.list, s.record);
        st.hip(hipGetLastError(), "kernel launch");
        return st.rc;
    });
    st.launch(k_corr_correlate, dim3(s.n_side, (s.n_side + 3) / 4), dim3(256), (const uint32_t *)s.list, g, (const uint32_t *)s.map, s.mp,
              (const int32_t *)s.table, s.n_side, (const int32_t *)s.record, s.surface);
    st.launch(k_corr_pick, dim3(1), dim3(1024), (const int32_t *)s.surface, s.n_side, s.record);
    int32_t rec[RELOC_CORR_RECORD_WORDS + 1] = {};
    st.download(rec, s.record, sizeof(rec));
    if (surface) st.download(surface, s.surface, (int64_t)s.n_side * s.n_side * 4);
    if (int rc = st.finish()) return rc;
    if (rec[RELOC_CORR_RECORD_WORDS] != 0) { reloc_set_error("correlation scan: %d cells fell outside the window", rec[RELOC_CORR_RECORD_WORDS]); return RELOC_E_CAPACITY; }
    memcpy(record, rec, RELOC_CORR_RECORD_WORDS * 4);
    return RELOC_OK;
}

RELOC_API int reloc_corr_match_points(reloc_ctx *ctx, const float *pts, int n, const double T12[12], double vio_x, double vio_y, int32_t *record,
                                      int32_t *surface)
{
    ARG_CHECK_CTX(ctx, n >= 0 && (pts || n == 0) && T12 && record, "reloc_corr_match_points");
    if (int rc = corr_check(ctx, T12, vio_x, vio_y, "reloc_corr_match_points")) return rc;
    HostStaging st{ctx};
    return corr_tick(ctx, st, frame_from_cloud(st, pts, n), T12, vio_x, vio_y, record, surface);
}

RELOC_API int reloc_corr_match_depth(reloc_ctx *ctx, const void *depth, int is_f32, int w, int h, int step, const double K4[4], float zmin, float zmax,
                                     const double T12[12], double vio_x, double vio_y, int32_t *record, int32_t *surface)
{
    ARG_CHECK_CTX(ctx, depth && w > 0 && h > 0 && step > 0 && K4 && T12 && record, "reloc_corr_match_depth");
    if (int rc = corr_check(ctx, T12, vio_x, vio_y, "reloc_corr_match_depth")) return rc;
    HostStaging st{ctx};
    return corr_tick(ctx, st, frame_from_depth(st, depth, is_f32, w, h, step, K4, zmin, zmax), T12, vio_x, vio_y, record, surface);
}

RELOC_API int reloc_corr_match_stereo_dev(reloc_ctx *ctx, int step, float zmin, float zmax, const double T12[12], double vio_x, double vio_y,
                                          int32_t *record, int32_t *surface)
{
    ARG_CHECK_CTX(ctx, step > 0 && T12 && record, "reloc_corr_match_stereo_dev");
    if (int rc = corr_check(ctx, T12, vio_x, vio_y, "reloc_corr_match_stereo_dev")) return rc;
    HostStaging st{ctx};
    return corr_tick(ctx, st, frame_from_stereo(st, step, zmin, zmax), T12, vio_x, vio_y, record, surface);
}

RELOC_API int reloc_corr_read_map(reloc_ctx *ctx, uint8_t *plane, int32_t *w, int32_t *h)
{
    ARG_CHECK_CTX(ctx, true, "reloc_corr_read_map");
    if (int rc = corr_need_map(ctx, "reloc_corr_read_map")) return rc;
    const CorrState &s = ctx->corr;
    if (w) *w = s.w;
    if (h) *h = s.h;
    if (!plane) return RELOC_OK;
    const int64_t cells = (int64_t)s.w * s.h;
    HostStaging st{ctx};
    uint8_t *d = st.slot<uint8_t>(6, cells);
    st.launch(k_corr_unpack, dim3(grid_1d(cells, 1024)), dim3(256), (const uint32_t *)s.map, d, s.w, s.h, s.mp);
    st.download(plane, d, cells);
    return st.finish();
}
