// reloc_route.hip -- route clearance (include/reloc_spec.h "ROUTE"; DESIGN.md "Route clearance").
// Once per map, on one bit per cell (bit b of word k = column 32 k + b, as the correlation map packs it: corr_pack_plane):
//   k_route_stamp      the stamps' rectangles OR-ed into the packed plane, a workgroup per rectangle
//   k_route_rows       a thread per word: the distance of its 32 cells to the nearest set bit of the same row, from leading /
//                      trailing zero counts on the word's own bits and on the words beside it, capped, 32 bytes out
//   k_route_cols       min over |dr| <= cap of row distance + |dr|, a thread per row and four columns, reading the 2 cap + 1
//                      rows of its cells (a sweep over row tiles with a cap-row halo was measured against it and lost at
//                      every cap: DESIGN.md "Route clearance")
// Per query:
//   k_route_gather     the clearance bytes at n cells
//   k_route_search     a wave per start cell, 64 table entries a round, ballot, the first round with a hit ends the wave
// Integers only; every plane of bytes has rows of ws = 32 * mp bytes, so a word of four cells is always aligned.
#include "reloc_teach.h"

constexpr int ROUTE_BIG = 1 << 20;             // "no occupied cell": beyond every cap, and sums of two never wrap

__global__ __launch_bounds__(256) void k_route_stamp(const int32_t *__restrict__ stamps, uint32_t *__restrict__ bits, int W, int H, int MP)
{
    const int32_t *s = stamps + 4 * blockIdx.x;
    const int r_lo = max(s[0], 0), r_hi = min(s[1], H), c_lo = max(s[2], 0), c_hi = min(s[3], W);
    if (r_hi <= r_lo || c_hi <= c_lo) return;
    const int k_lo = c_lo >> 5, nk = ((c_hi - 1) >> 5) - k_lo + 1, n = nk * (r_hi - r_lo);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int r = r_lo + i / nk, k = k_lo + i % nk;
        const int b_lo = max(c_lo - 32 * k, 0), b_hi = min(c_hi - 32 * k, 32);           // bits [b_lo, b_hi) of the word
        const uint32_t mask = (0xFFFFFFFFu >> (32 - (b_hi - b_lo))) << b_lo;
        atomicOr(&bits[r * MP + k], mask);
    }
}

__device__ __forceinline__ uint32_t route_byte(int d, int cap) { return d <= cap ? (uint32_t)d : (uint32_t)RELOC_ROUTE_FAR; }

__global__ __launch_bounds__(256) void k_route_rows(const uint32_t *__restrict__ bits, uint8_t *__restrict__ rowd, int H, int MP, int cap)
{
    const int n = H * MP;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += gridDim.x * blockDim.x) {
        const int k = idx % MP;
        const uint32_t *row = bits + (idx - k);
        const uint32_t w = row[k];
        // from bit 0 to the nearest set bit of the words before, from bit 31 to that of the words behind
        int left = ROUTE_BIG, right = ROUTE_BIG;
        for (int j = 1; j <= k && 32 * (j - 1) < cap; ++j)
            if (const uint32_t u = row[k - j]) { left = 32 * (j - 1) + __clz((int)u) + 1; break; }
        for (int j = 1; k + j < MP && 32 * (j - 1) < cap; ++j)
            if (const uint32_t u = row[k + j]) { right = 32 * (j - 1) + (__ffs((int)u) - 1) + 1; break; }
        uint32_t out[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            uint32_t v = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int b = 4 * q + t;
                const uint32_t lower = w & (0xFFFFFFFFu >> (31 - b)), upper = w >> b;
                const int dl = lower ? b - (31 - __clz((int)lower)) : b + left;
                const int dr = upper ? __ffs((int)upper) - 1 : 31 - b + right;
                v |= route_byte(min(dl, dr), cap) << (8 * t);
            }
            out[q] = v;
        }
        uint4 *dst = reinterpret_cast<uint4 *>(rowd + (size_t)idx * 32);
        dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
        dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
    }
}

// four cells of a byte plane as distances, RELOC_ROUTE_FAR as ROUTE_BIG
__device__ __forceinline__ void route_unpack(uint32_t v, int d[4])
{
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int b = (int)(v >> (8 * t) & 255u);
        d[t] = b == RELOC_ROUTE_FAR ? ROUTE_BIG : b;
    }
}

__device__ __forceinline__ uint32_t route_pack(const int d[4], int cap)
{
    return route_byte(d[0], cap) | route_byte(d[1], cap) << 8 | route_byte(d[2], cap) << 16 | route_byte(d[3], cap) << 24;
}

// a thread per row and four columns
__global__ __launch_bounds__(256) void k_route_cols(const uint32_t *__restrict__ rowd, uint32_t *__restrict__ clear, int H, int S, int cap)
{
    const int n = H * S;                          // S: words of four cells per row
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += gridDim.x * blockDim.x) {
        const int r = idx / S;
        int best[4] = {ROUTE_BIG, ROUTE_BIG, ROUTE_BIG, ROUTE_BIG};
        for (int rr = max(r - cap, 0); rr <= min(r + cap, H - 1); ++rr) {
            int d[4];
            route_unpack(rowd[idx + (rr - r) * S], d);
            const int a = abs(rr - r);
#pragma unroll
            for (int t = 0; t < 4; ++t) best[t] = min(best[t], d[t] + a);
        }
        clear[idx] = route_pack(best, cap);
    }
}

// (g) on unsigned sums: a start cell may be any int32, an offset is within RELOC_ROUTE_MAX_OFFSET, so a sum that wraps never
// lands inside a plane of at most 32768 cells a side
__device__ __forceinline__ bool route_inside(int at, int off, int n, int &out)
{
    const unsigned v = (unsigned)at + (unsigned)off;
    out = (int)v;
    return v < (unsigned)n;
}

__global__ __launch_bounds__(256) void k_route_gather(const uint8_t *__restrict__ clear, int W, int H, int WS, const int32_t *__restrict__ cells,
                                                      int n, uint8_t *__restrict__ out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int r = cells[2 * i], c = cells[2 * i + 1];
        out[i] = (unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W ? clear[r * WS + c] : (uint8_t)RELOC_ROUTE_FAR;
    }
}

// PRED = RELOC_ROUTE_PRED_CLEARANCE: plane = the clearance plane (rows of `stride` bytes), read at the remapped cell, >= thresh;
// RELOC_ROUTE_PRED_COST: plane = the int8 costmap, 0 <= cost < thresh
template <int PRED>
__global__ __launch_bounds__(256) void k_route_search(const void *__restrict__ plane, int W, int H, int stride, const int32_t *__restrict__ row_remap,
                                                      const int32_t *__restrict__ col_remap, int thresh, const int2 *__restrict__ table,
                                                      int n_off, const int2 *__restrict__ cells, int n, int32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));       // the wave's start cell: scalar loads
    if (i >= n) return;
    const int2 start = cells[i];
    int found = -1;
    for (int base = 0; base < n_off; base += 64) {
        const int k = base + lane;
        bool ok = false;
        if (k < n_off) {
            const int2 e = table[k];
            int r, c;
            if (route_inside(start.x, e.x, H, r) & route_inside(start.y, e.y, W, c)) {
                if (PRED == RELOC_ROUTE_PRED_CLEARANCE) {
                    ok = (int)reinterpret_cast<const uint8_t *>(plane)[row_remap[r] * stride + col_remap[c]] >= thresh;
                } else {
                    const int v = reinterpret_cast<const int8_t *>(plane)[r * stride + c];
                    ok = v >= 0 && v < thresh;
                }
            }
        }
        const unsigned long long hits = __ballot(ok);
        if (hits) { found = base + (__ffsll((long long)hits) - 1); break; }
    }
    if (lane == 0) out[i] = found;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static int route_capacity(int w, int h, const char *who)
{
    if (w > RELOC_ROUTE_MAX_SIDE || h > RELOC_ROUTE_MAX_SIDE || (int64_t)w * h > RELOC_OCC_MAX_CELLS) {
        reloc_set_error("%s: plane %d x %d exceeds the capacity (%d cells, %d per side)", who, w, h, RELOC_OCC_MAX_CELLS, RELOC_ROUTE_MAX_SIDE);
        return RELOC_E_CAPACITY;
    }
    return RELOC_OK;
}

// the checks that need no device, in the order of include/reloc.h: arguments first, then capacity
static int route_map_check(int w, int h, const int32_t *stamps, int n_stamps, int cap, const int32_t *row_remap, const int32_t *col_remap,
                           const char *who)
{
    if (cap < 0 || cap > RELOC_ROUTE_MAX_CAP) { reloc_set_error("bad argument: %s: cap %d outside [0, %d]", who, cap, RELOC_ROUTE_MAX_CAP); return RELOC_E_ARG; }
    for (int k = 0; k < n_stamps; ++k)
        if (stamps[4 * k] > stamps[4 * k + 1] || stamps[4 * k + 2] > stamps[4 * k + 3]) {
            reloc_set_error("bad argument: %s: stamp %d has lo > hi", who, k);
            return RELOC_E_ARG;
        }
    if (int rc = route_capacity(w, h, who)) return rc;
    for (int r = 0; row_remap && r < h; ++r)
        if ((unsigned)row_remap[r] >= (unsigned)h) { reloc_set_error("bad argument: %s: row_remap[%d] = %d lies outside the plane", who, r, row_remap[r]); return RELOC_E_ARG; }
    for (int c = 0; col_remap && c < w; ++c)
        if ((unsigned)col_remap[c] >= (unsigned)w) { reloc_set_error("bad argument: %s: col_remap[%d] = %d lies outside the plane", who, c, col_remap[c]); return RELOC_E_ARG; }
    return RELOC_OK;
}

// the block of a w x h map, grown when too small; a failure leaves the map before as it was, behind the layout it is gone
static int route_map_begin(reloc_ctx *ctx, int w, int h, int cap)
{
    RouteState &s = ctx->route;
    const int mp = (w + 31) / 32, ws = 32 * mp;
    if (int rc = s.block.layout(ctx, [&](BlockCarver &c) {
            c.aligned<16>(s.rowd, (int64_t)ws * h);      // rows of 32 bytes first: k_route_rows stores uint4
            c.aligned<16>(s.clear, (int64_t)ws * h);
            c(s.bits, (int64_t)mp * h);
            c(s.row_remap, h);
            c(s.col_remap, w);
        })) return rc;
    s.w = s.h = 0;
    s.mp = mp; s.ws = ws; s.cap = cap;
    return RELOC_OK;
}

// `plane` (device memory) -> bits -> stamps -> rows -> columns, and the remap tables (NULL: identity)
static int route_map_build(reloc_ctx *ctx, HostStaging &st, int w, int h, const void *plane, bool from_units, const int32_t *stamps, int n_stamps,
                           const int32_t *row_remap, const int32_t *col_remap)
{
    RouteState &s = ctx->route;
    const int cap = s.cap, S = s.ws / 4;
    const int64_t words = (int64_t)s.mp * h;
    corr_pack_plane(st, plane, from_units, s.bits, w, h, s.mp);
    if (n_stamps > 0)
        st.launch(k_route_stamp, dim3(n_stamps), dim3(256), (const int32_t *)st.upload_slot(5, stamps, (int64_t)n_stamps * 4), s.bits, w, h, s.mp);
    st.launch(k_route_rows, dim3(grid_1d(words, 4096)), dim3(256), (const uint32_t *)s.bits, s.rowd, h, s.mp, cap);
    st.launch(k_route_cols, dim3(grid_1d((int64_t)S * h, 4096)), dim3(256), (const uint32_t *)s.rowd, (uint32_t *)s.clear, h, S, cap);
    std::vector<int32_t> ident;
    if (!row_remap || !col_remap) {
        ident.resize(w > h ? w : h);
        for (int k = 0; k < (int)ident.size(); ++k) ident[k] = k;
    }
    st.upload(s.row_remap, row_remap ? row_remap : ident.data(), (int64_t)h * 4);
    st.upload(s.col_remap, col_remap ? col_remap : ident.data(), (int64_t)w * 4);
    const int rc = st.finish();                   // `ident` and the caller's arrays are read by then
    if (!rc) { s.w = w; s.h = h; }
    return rc;
}

RELOC_API int reloc_route_set_map(reloc_ctx *ctx, const uint8_t *occupied, int w, int h, const int32_t *stamps, int n_stamps, int cap,
                                  const int32_t *row_remap, const int32_t *col_remap)
{
    ARG_CHECK_CTX(ctx, occupied && w > 0 && h > 0 && n_stamps >= 0 && (stamps || n_stamps == 0),
                  "reloc_route_set_map: a plane, positive sizes, n_stamps >= 0 with their rectangles");
    if (int rc = route_map_check(w, h, stamps, n_stamps, cap, row_remap, col_remap, "reloc_route_set_map")) return rc;
    if (int rc = route_map_begin(ctx, w, h, cap)) return rc;
    HostStaging st{ctx};
    return route_map_build(ctx, st, w, h, st.upload_slot(6, occupied, (int64_t)w * h), false, stamps, n_stamps, row_remap, col_remap);
}

RELOC_API int reloc_route_set_map_from_occ(reloc_ctx *ctx, const int32_t *stamps, int n_stamps, int cap, const int32_t *row_remap,
                                           const int32_t *col_remap)
{
    ARG_CHECK_CTX(ctx, n_stamps >= 0 && (stamps || n_stamps == 0), "reloc_route_set_map_from_occ: n_stamps >= 0 with their rectangles");
    if (int rc = occ_need_map(ctx, "reloc_route_set_map_from_occ")) return rc;
    const OccState &o = ctx->occ;
    if (int rc = route_map_check(o.w, o.h, stamps, n_stamps, cap, row_remap, col_remap, "reloc_route_set_map_from_occ")) return rc;
    if (int rc = route_map_begin(ctx, o.w, o.h, cap)) return rc;
    HostStaging st{ctx};
    return route_map_build(ctx, st, o.w, o.h, o.units, true, stamps, n_stamps, row_remap, col_remap);
}

static int route_need_map(const reloc_ctx *ctx, const char *who) { return need_map(ctx->route.on(), who, "route", "reloc_route_set_map"); }

RELOC_API int reloc_route_read_clearance(reloc_ctx *ctx, uint8_t *plane, int32_t *w, int32_t *h)
{
    ARG_CHECK_CTX(ctx, true, "reloc_route_read_clearance");
    if (int rc = route_need_map(ctx, "reloc_route_read_clearance")) return rc;
    const RouteState &s = ctx->route;
    if (w) *w = s.w;
    if (h) *h = s.h;
    if (!plane) return RELOC_OK;
    HostStaging st{ctx};
    st.download_rows(plane, s.clear, s.w, s.h, s.ws);
    return st.finish();
}

RELOC_API int reloc_route_clearance_at(reloc_ctx *ctx, const int32_t *cells_rc, int n, uint8_t *out)
{
    ARG_CHECK_CTX(ctx, n >= 0 && ((cells_rc && out) || n == 0), "reloc_route_clearance_at: n >= 0 cells and their output");
    if (int rc = route_need_map(ctx, "reloc_route_clearance_at")) return rc;
    if (n == 0) return RELOC_OK;
    const RouteState &s = ctx->route;
    HostStaging st{ctx};
    const int32_t *cells = st.upload_slot(5, cells_rc, (int64_t)n * 2);
    uint8_t *d = st.slot<uint8_t>(6, n);
    st.launch(k_route_gather, dim3(grid_1d(n, 4096)), dim3(256), (const uint8_t *)s.clear, s.w, s.h, s.ws, cells, n, d);
    st.download(out, d, n);
    return st.finish();
}

RELOC_API int reloc_route_set_costmap(reloc_ctx *ctx, const int8_t *cost, int w, int h)
{
    ARG_CHECK_CTX(ctx, cost && w > 0 && h > 0, "reloc_route_set_costmap: a plane and positive sizes");
    if (int rc = route_capacity(w, h, "reloc_route_set_costmap")) return rc;
    RouteState &s = ctx->route;
    const int64_t bytes = (int64_t)w * h;
    if (int rc = s.cost.reserve(ctx, (size_t)bytes)) return rc;
    s.cw = s.ch = 0;
    HostStaging st{ctx};
    st.upload(s.cost.p, cost, bytes);
    const int rc = st.finish();
    if (!rc) { s.cw = w; s.ch = h; }
    return rc;
}

RELOC_API int reloc_route_search(reloc_ctx *ctx, int predicate, int thresh, const int32_t *offsets_rc, int n_offsets, const int32_t *cells_rc,
                                 int n, int32_t *out_index)
{
    ARG_CHECK_CTX(ctx, (predicate == RELOC_ROUTE_PRED_CLEARANCE || predicate == RELOC_ROUTE_PRED_COST) && n_offsets >= 0 && (offsets_rc || n_offsets == 0) &&
                           n >= 0 && ((cells_rc && out_index) || n == 0),
                  "reloc_route_search: a predicate RELOC_ROUTE_PRED_*, n_offsets >= 0 table entries, n >= 0 cells and their output");
    const RouteState &s = ctx->route;
    if (predicate == RELOC_ROUTE_PRED_CLEARANCE) {
        if (int rc = route_need_map(ctx, "reloc_route_search")) return rc;
    } else if (!s.has_cost()) {
        reloc_set_error("reloc_route_search: no costmap on this context (reloc_route_set_costmap)");
        return RELOC_E_STATE;
    }
    if (n_offsets > RELOC_ROUTE_MAX_OFFSETS) {
        reloc_set_error("reloc_route_search: %d table entries exceed the capacity (%d)", n_offsets, RELOC_ROUTE_MAX_OFFSETS);
        return RELOC_E_CAPACITY;
    }
    for (int k = 0; k < 2 * n_offsets; ++k)
        if (offsets_rc[k] > RELOC_ROUTE_MAX_OFFSET || offsets_rc[k] < -RELOC_ROUTE_MAX_OFFSET) {
            reloc_set_error("reloc_route_search: table entry %d reaches %d cells, beyond the capacity (%d)", k / 2, offsets_rc[k], RELOC_ROUTE_MAX_OFFSET);
            return RELOC_E_CAPACITY;
        }
    if (n == 0) return RELOC_OK;
    if (n_offsets == 0) {                         // an empty table has no first entry
        for (int i = 0; i < n; ++i) out_index[i] = -1;
        return RELOC_OK;
    }
    HostStaging st{ctx};
    const int2 *table = (const int2 *)st.upload_slot(5, offsets_rc, (int64_t)n_offsets * 2);
    const int2 *cells = (const int2 *)st.upload_slot(6, cells_rc, (int64_t)n * 2);
    int32_t *d = st.slot<int32_t>(7, n);
    const dim3 grid((n + 3) / 4), block(256);
    if (predicate == RELOC_ROUTE_PRED_CLEARANCE)
        st.launch(k_route_search<RELOC_ROUTE_PRED_CLEARANCE>, grid, block, (const void *)s.clear, s.w, s.h, s.ws, (const int32_t *)s.row_remap,
                  (const int32_t *)s.col_remap, thresh, table, n_offsets, cells, n, d);
    else
        st.launch(k_route_search<RELOC_ROUTE_PRED_COST>, grid, block, (const void *)s.cost.p, s.cw, s.ch, s.cw, (const int32_t *)nullptr,
                  (const int32_t *)nullptr, thresh, table, n_offsets, cells, n, d);
    st.download(out_index, d, (int64_t)n * 4);
    return st.finish();
}
