// reloc_orb.hip -- ORB front end on gfx950: gray -> 8-level pyramid -> FAST-9/16 + NMS ->
// best-2n by FAST score -> Harris -> best-n -> intensity-centroid angle -> 7x7 blur -> steered
// BRIEF-256.  Serves cv2.cvtColor(.., COLOR_BGR2GRAY) and
// cv2.ORB_create(nfeatures).detectAndCompute(gray, None)        (reference M:305-306, R:240-241).
//
// Everything is integer or strictly-ordered IEEE float arithmetic (no fused multiply-add, own
// sin/cos) so results are bit-identical to the specification; the algorithm constants live in
// include/reloc_spec.h.  Data layout in HBM: every pyramid level is a plane with a 64-byte-aligned
// row stride inside one arena (ctx->pyr); the blurred pyramid (ctx->blur) and the NMS score maps
// (ctx->nms) use the same geometry, so a level is addressed by one offset in all three.
//
// Launches per frame (all on the ctx stream):
//   k_pyramid                            gray conversion (or a gray plane) and all 8 levels in one launch: a tile
//                                        owns a rectangle of every level and derives level l from level l-1 in LDS
//                                        (fixed-point INTER_LINEAR_EXACT), 4 px per lane, dword stores
//   k_fast_blur                          one launch, two kinds of tiles over all levels, halos staged in LDS as aligned
//                                        dwords (a lane owns a fixed (row, dword); border bytes only in border tiles):
//                                        FAST 32x32 tiles: segment test of four adjacent pixels per lane on 7 x 3 LDS
//                                        dwords (v_perm_b32 + 16-bit sign arithmetic, two pixels per instruction), the
//                                        132 pixels of the ring around the tile one per lane; scores of the compacted
//                                        corners, 3x3 NMS, per-level score histogram (LDS atomics, then global);
//                                        blur 64x16 tiles: four horizontal sums per lane from three dwords
//                                        (v_alignbyte_b32 + two v_dot4_u32_u8 per window), vertical pass on 16-bit
//                                        pairs (8.8 / 16.16 passes)
//   k_harris                             histogram -> cut score; survivors >= cut get a Harris
//                                        response and enter the per-level candidate list
//   k_select                             one workgroup per level: keep "fewer than quota strictly
//                                        greater", order raster by rank counting
//   k_describe                           one wave per keypoint: moments by wave reduction, angle,
//                                        256 steered tests -> 4 ballots = 32 descriptor bytes
// The per-frame HBM traffic is about 4 MB at 640x480; the stage is launch/latency-bound, not
// bandwidth-bound.
#include <float.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "../../include/reloc_orb_pattern.h"
#include "reloc_internal.h"

typedef uint32_t u32;

constexpr int HARRIS_CHUNK = 1024;   // bytes of the NMS map per k_harris block (4 per thread)
static_assert(HARRIS_CHUNK == 1024, "k_harris reads one dword per thread");

struct OrbTable {
    OrbLevel lev[NLEV];
    int fast_tile_base[NLEV + 1];   // 32x32 tiles over (stride x h)
    int blur_tile_base[NLEV + 1];   // 64x16 tiles over (w x h)
    int flat_base[NLEV + 1];        // HARRIS_CHUNK-byte chunks over stride*h
    int rz_off[NLEV][4];            // offsets into the resize table: xofs, xcoef, yofs, ycoef
};

__constant__ signed char c_pattern[RELOC_ORB_NTESTS * 4];
__constant__ int c_umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
__constant__ signed char c_ring_dx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
__constant__ signed char c_ring_dy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};

__device__ __forceinline__ int find_level(const int *base, int id)
{
    int l = 0;
#pragma unroll
    for (int k = 1; k < NLEV; ++k) l += id >= base[k];
    return l;
}

__device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) {
        if (p < 0) p = -p;
        if (p >= n) p = 2 * n - 2 - p;
    }
    return p;
}

// ---- gray ---------------------------------------------------------------------------------------
// `order_rgb` of the gray stages carries two flags: bit 0 = RELOC_ORDER_RGB, bit 1 = RELOC_GRAY_FLAG_15BIT (the 15-bit
// coefficient set of reloc_params.gray_coeff_bits == 15).  Both are launch-uniform: the selects run on the scalar unit.
__device__ __forceinline__ int gray_fixed(int b, int g, int r, int flags)
{
    const bool c15 = flags & RELOC_GRAY_FLAG_15BIT;
    const int cb = c15 ? RELOC_GRAY15_CB : RELOC_GRAY_CB, cg = c15 ? RELOC_GRAY15_CG : RELOC_GRAY_CG, cr = c15 ? RELOC_GRAY15_CR : RELOC_GRAY_CR;
    const int sh = c15 ? RELOC_GRAY15_SHIFT : RELOC_GRAY_SHIFT;
    return (b * cb + g * cg + r * cr + (1 << (sh - 1))) >> sh;
}
static inline int gray_flags(const reloc_ctx *ctx, int order)
{
    return (order & 1) | (ctx->prm.gray_coeff_bits == RELOC_GRAY15_SHIFT ? RELOC_GRAY_FLAG_15BIT : 0);
}
// plain gray output for reloc_gray_u8 (dense rows)
__global__ __launch_bounds__(256) void k_gray_plain(const uint8_t *__restrict__ src, int w, int h, int sstride, int order_rgb,
                                                    uint8_t *__restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const uint8_t *s = src + (size_t)y * sstride + 3 * x;
    const int c0 = s[0], c1 = s[1], c2 = s[2];
    const int b = (order_rgb & 1) ? c2 : c0, r = (order_rgb & 1) ? c0 : c2;
    dst[(size_t)y * w + x] = (uint8_t)gray_fixed(b, c1, r, order_rgb);
}

// ---- fused pyramid ------------------------------------------------------------------------------
// One launch builds level 0 (gray conversion or a copy of a gray plane) AND levels 1..7.  Level l is a
// resize of level l-1; as seven launches (round 1) that was a dependent chain of tiny kernels, 4.3 us
// each, 30 us of a 75 us front end.  Here a workgroup owns one rectangle of EVERY level (`o`, 4-pixel
// aligned in x so it is stored as dwords) and computes, in LDS, the slightly larger rectangle `n` of
// each level that its rectangles of the levels above need as bilinear taps -- at most one extra
// row/column per level, so about 2x recomputation at level 0 and less above.  Per pixel the arithmetic
// is that of a plain per-level resize (same tables, same order), so the planes are bit-identical.  The rectangles and the
// table slices are worked out by the host once per frame size (orb_prepare).
#ifndef PYR_TW
#define PYR_TW 64
#define PYR_TH 32
#endif
constexpr int PT_W = PYR_TW, PT_H = PYR_TH;     // level-0 footprint of a tile
struct PyrTile {
    uint16_t o[NLEV][4];    // stored rectangle x0, x1, y0, y1 (x0 multiple of 4; x1 may reach into the row padding)
    uint16_t n[NLEV][4];    // computed rectangle (x0 multiple of 4, x1 <= level width)
};
static_assert(sizeof(PyrTile) == 128, "PyrTile is read as 8 dwordx4");

struct PyrLds { int lev[NLEV]; int tabs; };    // byte offsets of the level buffers and of the table slices in LDS

// Frame-batched launches (reloc_tick_batch_dev, the sharded halves): the five ORB kernels of up to 8 contexts as FIVE
// launches, blockIdx.y = frame.  Everything a kernel needs of one context travels in the kernel arguments.
struct OrbFrame {
    const OrbTable *tab; const PyrTile *tiles; const int32_t *rz; const uint8_t *src;
    uint8_t *pyr, *nms, *blur; int32_t *hist, *cand_cnt; u32 *cand_key; float *cand_resp; int32_t *dbg_cut;
    int32_t *kp_cnt; u32 *kp_key; float *kp_resp; float *f_xy, *f_size, *f_angle, *f_resp; int32_t *f_oct; uint8_t *f_desc;
    int32_t *f_count;
};
struct OrbBatch { OrbFrame f[RELOC_BATCH_MAX]; };

// gray value of 4 pixels from 12 interleaved bytes / a gray dword
template <int CH, bool ALIGNED>
__device__ __forceinline__ void pyr_fetch(const uint8_t *sp, int x4, int w, u32 (&d)[3])
{
    if (ALIGNED) {
        const u32 *s4 = reinterpret_cast<const u32 *>(sp);
        d[0] = s4[0];
        if (CH == 3) { d[1] = s4[1]; d[2] = s4[2]; }
    } else {
        d[0] = d[1] = d[2] = 0;
#pragma unroll
        for (int k = 0; k < 4 * CH; ++k)
            if (x4 + k / CH < w) d[k >> 2] |= (u32)sp[k] << (8 * (k & 3));
    }
}

template <int CH>
__device__ __forceinline__ u32 pyr_gray4(const u32 (&d)[3], int x4, int w, int order_rgb)
{
    if (CH == 1) return d[0];     // bytes beyond w are 0 (unaligned fetch) or do not exist (aligned: w % 4 == 0)
    u32 out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int c[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { const int bi = 3 * k + j; c[j] = (d[bi >> 2] >> (8 * (bi & 3))) & 0xFF; }
        const int b = (order_rgb & 1) ? c[2] : c[0], r = (order_rgb & 1) ? c[0] : c[2];
        const int g = gray_fixed(b, c[1], r, order_rgb);
        if (x4 + k < w) out |= (u32)g << (8 * k);
    }
    return out;
}

// flat table index i -> positions of the (offset, coefficient) entries in the resize tables; the level is found
// by selects over uniform values so that no load depends on it
__device__ __forceinline__ void pyr_tab_index(const OrbTable *__restrict__ tab, const PyrTile &T, const int (&tbase)[NLEV + 1], int i,
                                              int &po, int &pc)
{
    int j = i, nw = 0, x0 = 0, y0 = 0, ox = 0, cx = 0, oy = 0, cy = 0;
#pragma unroll
    for (int k = 1; k < NLEV; ++k) {
        const bool m = i >= tbase[k];
        j = m ? i - tbase[k] : j;
        nw = m ? T.n[k][1] - T.n[k][0] : nw;
        x0 = m ? (int)T.n[k][0] : x0;
        y0 = m ? (int)T.n[k][2] : y0;
        ox = m ? tab->rz_off[k][0] : ox;
        cx = m ? tab->rz_off[k][1] : cx;
        oy = m ? tab->rz_off[k][2] : oy;
        cy = m ? tab->rz_off[k][3] : cy;
    }
    const bool isx = j < nw;
    const int p = isx ? x0 + j : y0 + j - nw;
    po = (isx ? ox : oy) + p;
    pc = (isx ? cx : cy) + p;
}

// q / d for the small quad counts of a tile (q < 2^16, d <= 2^8): exact through one float multiply
__device__ __forceinline__ int pyr_div(int q, float inv) { return (int)(((float)q + 0.5f) * inv); }

// PYR_BS = threads per workgroup: 512 is the fastest alone (256 / 512 / 1024: ORB stage 73 / 68 / 66 us), 256 the best
// neighbour of a scan (a 256-thread workgroup fits into the slot one retiring scan workgroup frees: 4-stream run 6550 ->
// 6685 frames/s, synchronous tick +6 us), so both exist: see orb_run.
template <int CH, bool ALIGNED, int PYR_BS>
__device__ __forceinline__ void pyramid_body(const OrbTable *__restrict__ tab, const PyrTile *__restrict__ tiles,
                                                 const int32_t *__restrict__ rz, const uint8_t *__restrict__ src, int w, int h,
                                                 int sstride, int order_rgb, uint8_t *__restrict__ pyr, PyrLds lds,
                                                 int32_t *__restrict__ hist, int32_t *__restrict__ cand_cnt)
{
    extern __shared__ u32 s_pyr[];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        for (int i = tid; i < NLEV * 256; i += PYR_BS) hist[i] = 0;
        if (tid < NLEV) cand_cnt[tid] = 0;
    }
    const PyrTile &T = tiles[blockIdx.x];
    uint8_t *const base = reinterpret_cast<uint8_t *>(s_pyr);
    u32 *const tabs = s_pyr + (lds.tabs >> 2);
    // ---- phase A: every global read of the tile, issued before anything waits ---------------------
    // table slices of the levels this tile touches, one flat index over (level, x | y): offset | coefficient << 16
    int tbase[NLEV + 1];
    tbase[1] = 0;
#pragma unroll
    for (int l = 1; l < NLEV; ++l) tbase[l + 1] = tbase[l] + (T.n[l][1] - T.n[l][0]) + (T.n[l][3] - T.n[l][2]);
    constexpr int TAB_IT = 1024 / PYR_BS, L0_IT = 1536 / PYR_BS;
    u32 tv[TAB_IT][2];
#pragma unroll
    for (int it = 0; it < TAB_IT; ++it) {
        const int i = tid + it * PYR_BS;
        tv[it][0] = tv[it][1] = 0;
        if (i < tbase[NLEV]) {
            int po, pc;
            pyr_tab_index(tab, T, tbase, i, po, pc);
            tv[it][0] = (u32)rz[po];
            tv[it][1] = (u32)rz[pc];
        }
    }
    const int x00 = T.n[0][0], y00 = T.n[0][2], qpr0 = (T.n[0][1] - x00 + 3) >> 2, nq0 = qpr0 * (T.n[0][3] - y00);
    const float inv0 = 1.0f / (float)(qpr0 > 0 ? qpr0 : 1);
    u32 fv[L0_IT][3];
#pragma unroll
    for (int it = 0; it < L0_IT; ++it) {
        const int q = tid + it * PYR_BS;
        if (q < nq0) {
            const int ry = pyr_div(q, inv0), x4 = x00 + (q - ry * qpr0) * 4;
            pyr_fetch<CH, ALIGNED>(src + (size_t)(y00 + ry) * sstride + CH * x4, x4, w, fv[it]);
        }
    }
#pragma unroll
    for (int it = 0; it < TAB_IT; ++it) {
        const int i = tid + it * PYR_BS;
        if (i < tbase[NLEV]) tabs[i] = tv[it][0] | tv[it][1] << 16;
    }
#pragma unroll
    for (int it = 0; it < L0_IT; ++it) {
        const int q = tid + it * PYR_BS;
        if (q < nq0) {
            const int ry = pyr_div(q, inv0), x4 = x00 + (q - ry * qpr0) * 4;
            reinterpret_cast<u32 *>(base + lds.lev[0])[q] = pyr_gray4<CH>(fv[it], x4, w, order_rgb);      // pitch = 4 * qpr0
        }
    }
    for (int q = tid + L0_IT * PYR_BS; q < nq0; q += PYR_BS) {        // larger tiles than planned for: plain loop
        const int ry = pyr_div(q, inv0), x4 = x00 + (q - ry * qpr0) * 4;
        u32 d[3];
        pyr_fetch<CH, ALIGNED>(src + (size_t)(y00 + ry) * sstride + CH * x4, x4, w, d);
        reinterpret_cast<u32 *>(base + lds.lev[0])[q] = pyr_gray4<CH>(d, x4, w, order_rgb);
    }
    for (int i = tid + TAB_IT * PYR_BS; i < tbase[NLEV]; i += PYR_BS) {
        int po, pc;
        pyr_tab_index(tab, T, tbase, i, po, pc);
        tabs[i] = (u32)rz[po] | (u32)rz[pc] << 16;
    }
    __syncthreads();
    // ---- phase B: levels 1..7 in LDS, each in its own buffer -----------------------------------------
#pragma unroll
    for (int l = 0; l + 1 < NLEV; ++l) {
        const int sw = tab->lev[l].w, sh = tab->lev[l].h;
        const uint8_t *cur = base + lds.lev[l];
        u32 *nxt = reinterpret_cast<u32 *>(base + lds.lev[l + 1]);
        const int nx0 = T.n[l][0], ny0 = T.n[l][2], pitch = ((T.n[l][1] - nx0 + 3) >> 2) << 2;
        const int dx0 = T.n[l + 1][0], dx1 = T.n[l + 1][1], dh = T.n[l + 1][3] - T.n[l + 1][2];
        const int qpr = (dx1 - dx0 + 3) >> 2;
        const u32 *xt = tabs + tbase[l + 1], *yt = xt + (dx1 - dx0);
        const u32 one = 1u << RELOC_RESIZE_COEF_BITS;
        const float inv = 1.0f / (float)(qpr > 0 ? qpr : 1);
        for (int q = tid; q < qpr * dh; q += PYR_BS) {
            const int ry = pyr_div(q, inv), rx4 = (q - ry * qpr) * 4;
            const u32 ye = yt[ry];
            const int sy0 = (int)(ye & 0xFFFF), sy1 = sy0 + 1 < sh ? sy0 + 1 : sh - 1;
            const u32 b = ye >> 16;
            const uint8_t *r0 = cur + (sy0 - ny0) * pitch - nx0, *r1 = cur + (sy1 - ny0) * pitch - nx0;
            u32 out = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (dx0 + rx4 + k < dx1) {
                    const u32 xe = xt[rx4 + k];
                    const int k0 = (int)(xe & 0xFFFF), k1 = k0 + 1 < sw ? k0 + 1 : sw - 1;
                    const u32 a = xe >> 16;
                    const u32 h0 = (u32)r0[k0] * (one - a) + (u32)r0[k1] * a;
                    const u32 h1 = (u32)r1[k0] * (one - a) + (u32)r1[k1] * a;
                    const u32 v = h0 * (one - b) + h1 * b;
                    out |= ((v + (1u << 15)) >> 16) << (8 * k);
                }
            }
            nxt[q] = out;      // pitch = 4 * qpr
        }
        __syncthreads();
    }
    // ---- phase C: every level's own rectangle to HBM, nothing waits on these stores -------------------
#pragma unroll
    for (int l = 0; l < NLEV; ++l) {
        const OrbLevel L = tab->lev[l];
        const uint8_t *cur = base + lds.lev[l];
        const int nx0 = T.n[l][0], ny0 = T.n[l][2], pitch = ((T.n[l][1] - nx0 + 3) >> 2) << 2;
        const int x0 = T.o[l][0], x1 = T.o[l][1], y0 = T.o[l][2], oh = T.o[l][3] - y0;
        const int qpr = (x1 - x0) >> 2;
        uint8_t *dst = pyr + L.off;
        const float inv = 1.0f / (float)(qpr > 0 ? qpr : 1);
        for (int q = tid; q < qpr * oh; q += PYR_BS) {
            const int ry = pyr_div(q, inv), x4 = x0 + (q - ry * qpr) * 4;
            u32 v = 0;
            if (x4 < L.w) {
                v = *reinterpret_cast<const u32 *>(cur + (y0 + ry - ny0) * pitch + (x4 - nx0));
                if (x4 + 4 > L.w) v &= 0xFFFFFFFFu >> (8 * (x4 + 4 - L.w));
            }
            *reinterpret_cast<u32 *>(dst + (size_t)(y0 + ry) * L.stride + x4) = v;
        }
    }
}
template <int CH, bool ALIGNED, int PYR_BS>
__global__ __launch_bounds__(PYR_BS) void k_pyramid(const OrbTable *__restrict__ tab, const PyrTile *__restrict__ tiles,
                                                 const int32_t *__restrict__ rz, const uint8_t *__restrict__ src, int w, int h,
                                                 int sstride, int order_rgb, uint8_t *__restrict__ pyr, PyrLds lds,
                                                 int32_t *__restrict__ hist, int32_t *__restrict__ cand_cnt)
{
    RELOC_SMALL_KERNEL_PRIO();
    pyramid_body<CH, ALIGNED, PYR_BS>(tab, tiles, rz, src, w, h, sstride, order_rgb, pyr, lds, hist, cand_cnt);
}
template <int CH, bool ALIGNED, int PYR_BS>
__global__ __launch_bounds__(PYR_BS) void k_pyramid_batch(OrbBatch b, int w, int h, int sstride, int order_rgb, PyrLds lds)
{
    RELOC_SMALL_KERNEL_PRIO();
    const OrbFrame &F = b.f[blockIdx.y];
    pyramid_body<CH, ALIGNED, PYR_BS>(F.tab, F.tiles, F.rz, F.src, w, h, sstride, order_rgb, F.pyr, lds, F.hist, F.cand_cnt);
}


// ---- blur ---------------------------------------------------------------------------------------
// Four bytes of one level row starting at the 4-aligned column gx, with the border rule applied per byte (BORDER_REFLECT_101
// for the blur, clamp for FAST).  A dword that lies inside the image is one aligned load: rows start 64-byte aligned.
template <bool REFLECT>
__device__ __forceinline__ u32 halo_dword(const uint8_t *__restrict__ row, int gx, int w)
{
    if (gx >= 0 && gx + 4 <= w) return *reinterpret_cast<const u32 *>(row + gx);
    u32 v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = REFLECT ? reflect101(gx + k, w) : min(max(gx + k, 0), w - 1);
        v |= (u32)row[x] << (8 * k);
    }
    return v;
}

constexpr int BT_W = 64, BT_H = 16;
constexpr int BT_P = BT_W / 4 + 2;      // dwords per staged row: columns x0 - 4 .. x0 + BT_W + 3
static_assert(BT_W == 64 && BT_H == 16, "blur7_tile maps 256 lanes to 16 rows x 16 dwords");
__device__ __forceinline__ void blur7_tile(const OrbTable *__restrict__ tab, const uint8_t *__restrict__ pyr,
                                           uint8_t *__restrict__ blur, int bid)
{
    __shared__ u32 s_in[(BT_H + 6) * BT_P];
    __shared__ u32 s_h[(BT_H + 6) * BT_W / 2];      // horizontal sums, two 16-bit values per dword
    const int l = find_level(tab->blur_tile_base, bid);
    const OrbLevel L = tab->lev[l];
    const int tile = bid - tab->blur_tile_base[l];
    const int tx = (L.w + BT_W - 1) / BT_W;
    const int x0 = (tile % tx) * BT_W, y0 = (tile / tx) * BT_H;
    const uint8_t *src = pyr + L.off;
    const int tid = threadIdx.x;
    const int r16 = tid >> 4, c16 = tid & 15;
    // halo: a lane owns one dword of one row.  Trip A: rows 0..15, the 16 dwords of the tile's own columns.  Trip B: lanes
    // 0..95 the same for rows 16..21, lanes 96..139 the dword left and right of the tile for all 22 rows.
    {
        const int e = tid - 6 * 16;
        const bool edge = e >= 0;
        const int rb = edge ? e >> 1 : BT_H + r16, db = edge ? (e & 1) * (BT_P - 1) : 1 + c16;
        const bool on = e < 2 * (BT_H + 6);
        const int gya = reflect101(y0 + r16 - 3, L.h), gyb = reflect101(y0 + rb - 3, L.h);
        const u32 va = halo_dword<true>(src + (size_t)gya * L.stride, x0 + 4 * c16, L.w);
        u32 vb = 0;
        if (on) vb = halo_dword<true>(src + (size_t)gyb * L.stride, x0 - 4 + 4 * db, L.w);
        s_in[r16 * BT_P + 1 + c16] = va;
        if (on) s_in[rb * BT_P + db] = vb;
    }
    __syncthreads();
    // horizontal pass: four adjacent sums from three dwords; a 7-tap window is two byte dot products (the taps fit a byte,
    // the sum 16 bits)
    constexpr u32 W_LO = RELOC_BLUR_K0 | RELOC_BLUR_K1 << 8 | RELOC_BLUR_K2 << 16 | (u32)RELOC_BLUR_K3 << 24;
    constexpr u32 W_HI = RELOC_BLUR_K2 | RELOC_BLUR_K1 << 8 | RELOC_BLUR_K0 << 16;
    static_assert(RELOC_BLUR_K3 < 256 && 2 * (RELOC_BLUR_K0 + RELOC_BLUR_K1 + RELOC_BLUR_K2) + RELOC_BLUR_K3 <= 256, "blur taps");
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int ry = t * BT_H + r16;
        if (ry < BT_H + 6) {
            const u32 *p = s_in + ry * BT_P + c16;
            const u32 d0 = p[0], d1 = p[1], d2 = p[2];      // columns x0 + 4 * c16 - 4 .. + 7
            u32 s[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {                   // output k: bytes 1 + k .. 7 + k
                const u32 lo = k < 3 ? __builtin_amdgcn_alignbyte(d1, d0, 1 + k) : d1;
                const u32 hi = k < 3 ? __builtin_amdgcn_alignbyte(d2, d1, 1 + k) : d2;
                s[k] = __builtin_amdgcn_udot4(lo, W_LO, __builtin_amdgcn_udot4(hi, W_HI, 0u, false), false);
            }
            *reinterpret_cast<uint2 *>(s_h + ry * (BT_W / 2) + 2 * c16) = make_uint2(s[0] | s[1] << 16, s[2] | s[3] << 16);
        }
    }
    __syncthreads();
    // vertical pass: 4 output pixels per lane, the seven rows read as 16-bit pairs
    {
        u32 c[7][4];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const uint2 d = *reinterpret_cast<const uint2 *>(s_h + (r16 + j) * (BT_W / 2) + 2 * c16);
            c[j][0] = d.x & 0xFFFF; c[j][1] = d.x >> 16; c[j][2] = d.y & 0xFFFF; c[j][3] = d.y >> 16;
        }
        u32 out = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32 s = RELOC_BLUR_K0 * (c[0][k] + c[6][k]) + RELOC_BLUR_K1 * (c[1][k] + c[5][k]) +
                          RELOC_BLUR_K2 * (c[2][k] + c[4][k]) + RELOC_BLUR_K3 * c[3][k];
            out |= ((s + (1u << 15)) >> 16) << (8 * k);
        }
        const int gy = y0 + r16, gx = x0 + 4 * c16;
        if (gy < L.h && gx < L.stride) *reinterpret_cast<u32 *>(blur + L.off + (size_t)gy * L.stride + gx) = out;
    }
}

// ---- FAST + NMS ---------------------------------------------------------------------------------
// segment test: 0 = not a corner, +1 = 9 contiguous brighter, -1 = 9 contiguous darker ring pixels
__device__ int fast_is_corner(const uint8_t *p, int stride, int thr)
{
    const int c = p[0];
    u32 bright = 0, dark = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int v = (int)p[c_ring_dy[k] * stride + c_ring_dx[k]] - c;
        bright |= (u32)(v > thr) << k;
        dark |= (u32)(v < -thr) << k;
    }
    // 9 contiguous set bits on the 16-bit circle
    auto run9 = [](u32 m) {
        u32 x = m | (m << 16);
        u32 y = x & (x >> 1);
        y &= y >> 2;
        y &= y >> 4;          // runs of 8
        y &= x >> 8;          // runs of 9
        return (y & 0xFFFFu) != 0;
    };
    return run9(bright) ? 1 : (run9(dark) ? -1 : 0);
}

// corner score of a pixel that passed the segment test with polarity `sign`: the largest threshold it still
// passes, i.e. max over the 16 arcs of 9 of the arc's minimum |difference|, minus 1
__device__ int fast_corner_score(const uint8_t *p, int stride, int thr, int sign)
{
    const int c = p[0];
    int v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = sign * ((int)p[c_ring_dy[k] * stride + c_ring_dx[k]] - c);
    int m2[16], m4[16], best = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) m2[k] = min(v[k], v[(k + 1) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) m4[k] = min(m2[k], m2[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int m8 = min(m4[k], m4[(k + 4) & 15]);
        const int m9 = min(m8, v[(k + 8) & 15]);
        best = max(best, m9);
    }
    return best > thr ? best - 1 : 0;
}

// 9 contiguous set bits on the 16-bit circle; x = the mask in both halves of a dword
__device__ __forceinline__ bool fast_run9(u32 x)
{
    u32 y = x & (x >> 1);
    y &= y >> 2;
    y &= y >> 4;          // runs of 8
    y &= x >> 8;          // runs of 9
    return (y & 0xFFFFu) != 0;
}

// Segment test of four horizontally adjacent pixels by one lane.  w[r][0..2] = the 12 bytes of row r (dy = r - 3) that start
// 4 columns left of pixel 0.  The ring byte (dx, dy) of the four pixels is four adjacent bytes of a row: one v_perm_b32 puts
// those of pixels 0 / 2 and one those of pixels 1 / 3 into 16-bit halves, where "brighter than centre + t" and "darker than
// centre - t" are the sign bits of one add / subtract for two pixels at a time.  The sign bits of the 16 ring positions are
// shifted into one 16-bit mask per pixel and polarity (mb / md: [0] = pixels 0 | 2 << 16, [1] = pixels 1 | 3 << 16).
struct FastQuad {
    u32 nb[2], nd[2];
    const u32 (*w)[3];
    __device__ __forceinline__ FastQuad(const u32 (&rows)[7][3]) : w(rows)
    {
        const u32 c = rows[3][1];
        const u32 ce = c & 0x00FF00FFu, co = (c >> 8) & 0x00FF00FFu;
        // v > c + t  <=>  v + (0x7FFF - c - t) has bit 15;   v < c - t  <=>  (c - t - 1 + 0x8000) - v has bit 15
        nb[0] = (0x7FFFu - RELOC_FAST_THRESHOLD) * 0x00010001u - ce; nb[1] = (0x7FFFu - RELOC_FAST_THRESHOLD) * 0x00010001u - co;
        nd[0] = (0x7FFFu - RELOC_FAST_THRESHOLD) * 0x00010001u + ce; nd[1] = (0x7FFFu - RELOC_FAST_THRESHOLD) * 0x00010001u + co;
    }
    // sign words of ring position (dx, dy): bit 15 of each half = the flag, the other bits are to be ignored
    template <int DX, int DY>
    __device__ __forceinline__ void flags(u32 (&tb)[2], u32 (&td)[2]) const
    {
        constexpr int b = 4 + DX, q = b >> 2, o = b & 3;
        constexpr u32 sel_e = (u32)o | 0x0C00u | (u32)(o + 2) << 16 | 0x0C000000u;
        constexpr u32 sel_o = (u32)(o + 1) | 0x0C00u | (u32)(o + 3) << 16 | 0x0C000000u;
        const u32 ve = __builtin_amdgcn_perm(w[DY + 3][q + 1], w[DY + 3][q], sel_e);
        const u32 vo = __builtin_amdgcn_perm(w[DY + 3][q + 1], w[DY + 3][q], sel_o);
        tb[0] = ve + nb[0]; tb[1] = vo + nb[1];
        td[0] = nd[0] - ve; td[1] = nd[1] - vo;
    }
    template <int K>
    __device__ __forceinline__ void ring(u32 (&tb)[2], u32 (&td)[2]) const
    {
        constexpr int dx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
        constexpr int dy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
        flags<dx[K], dy[K]>(tb, td);
    }
    // compass pretest: some pixel of the four has two brighter or two darker compass pixels
    __device__ __forceinline__ bool candidate() const
    {
        u32 b0[2], d0[2], b4[2], d4[2], b8[2], d8[2], b12[2], d12[2];
        ring<0>(b0, d0); ring<4>(b4, d4); ring<8>(b8, d8); ring<12>(b12, d12);
        u32 any = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            any |= (b0[j] & b4[j]) | (b8[j] & b12[j]) | ((b0[j] | b4[j]) & (b8[j] | b12[j]));
            any |= (d0[j] & d4[j]) | (d8[j] & d12[j]) | ((d0[j] | d4[j]) & (d8[j] | d12[j]));
        }
        return (any & 0x80008000u) != 0;
    }
    template <int K>
    __device__ __forceinline__ void shift_in(u32 (&mb)[2], u32 (&md)[2]) const
    {
        u32 tb[2], td[2];
        ring<K>(tb, td);
#pragma unroll
        for (int j = 0; j < 2; ++j) {      // ring position K ends at bit K of its half; what crosses the halves is overwritten
            mb[j] = (tb[j] & 0x80008000u) | ((mb[j] >> 1) & 0x7FFF7FFFu);
            md[j] = (td[j] & 0x80008000u) | ((md[j] >> 1) & 0x7FFF7FFFu);
        }
        if constexpr (K < 15) shift_in<K + 1>(mb, md);
    }
    __device__ __forceinline__ void masks(u32 (&mb)[2], u32 (&md)[2]) const
    {
        mb[0] = mb[1] = md[0] = md[1] = 0;
        shift_in<0>(mb, md);
    }
};

constexpr int FT = 32;
constexpr int FT_P = FT / 4 + 3;       // dwords per staged row: columns x0 - 4 .. x0 + FT + 3, one of padding
static_assert(FT == 32, "fast_nms_tile maps 256 lanes to 32 rows x 8 dwords");
__device__ __forceinline__ void fast_nms_tile(const OrbTable *__restrict__ tab, const uint8_t *__restrict__ pyr,
                                              uint8_t *__restrict__ nms, int32_t *__restrict__ hist, int bid)
{
    __shared__ u32 s_img4[(FT + 8) * FT_P];
    __shared__ u32 s_sc4[(FT + 2) * (FT + 4) / 4];
    __shared__ unsigned short s_corner[(FT + 2) * (FT + 2)];
    __shared__ int s_nc;
    __shared__ int s_hist[256];
    const uint8_t *const s_img = reinterpret_cast<const uint8_t *>(s_img4);
    uint8_t *const s_sc = reinterpret_cast<uint8_t *>(s_sc4);
    const int l = find_level(tab->fast_tile_base, bid);
    const OrbLevel L = tab->lev[l];
    const int tile = bid - tab->fast_tile_base[l];
    const int tx = L.stride / FT;
    const int x0 = (tile % tx) * FT, y0 = (tile / tx) * FT;
    const int tid = threadIdx.x;
    const int e = RELOC_ORB_EDGE;
    uint8_t *out = nms + L.off;
    // tiles that cannot hold a kept corner only clear their part of the map
    const bool live = L.quota > 0 && x0 + FT > e && x0 < L.w - e && y0 + FT > e && y0 < L.h - e;
    if (!live) {
        const int y = y0 + tid / 8, x = x0 + (tid % 8) * 4;
        if (y < L.h) *reinterpret_cast<u32 *>(out + (size_t)y * L.stride + x) = 0;
        return;
    }
    s_hist[tid] = 0;
    const uint8_t *src = pyr + L.off;
    const int IS = 4 * FT_P;
    // halo, clamped at the image border: a lane owns one dword of a row, 16 rows per trip (10 of 16 lanes load)
    {
        const int r16 = tid >> 4, c16 = tid & 15;
        u32 v[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int ry = 16 * t + r16;
            if (c16 < FT / 4 + 2 && ry < FT + 8) {
                const int gy = min(max(y0 + ry - 4, 0), L.h - 1);
                v[t] = halo_dword<false>(src + (size_t)gy * L.stride, x0 - 4 + 4 * c16, L.w);
            }
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int ry = 16 * t + r16;
            if (c16 < FT / 4 + 2 && ry < FT + 8) s_img4[ry * FT_P + c16] = v[t];
        }
    }
    for (int i = tid; i < (FT + 2) * (FT + 4) / 4; i += 256) s_sc4[i] = 0;
    if (tid == 0) s_nc = 0;
    __syncthreads();
    // segment test for every pixel of the tile + 1-px ring; the few corners are compacted into a list so that
    // the score (as long as the test itself) runs on full waves of corners instead of on every wave that
    // happens to contain one.  (Compacting the pretest survivors as well, so that the segment test too runs on full waves:
    // 21 % fewer instructions and no faster -- profiles/README.md "Dropped experiments" #7.)
    // The usual compass pretest, as a WAVE decision: an arc of 9 of the 16 ring pixels contains at least two of the four
    // compass pixels (ring positions 0, 4, 8, 12), so a pixel with fewer than two brighter and fewer than two darker
    // compass pixels is no corner.  Lanes cannot skip work on their own, but a wave whose pixels all fail (flat
    // ground, sky, the inside of uniform shapes) skips the 16-pixel segment test altogether; the outcome is the same.
    const int SS = FT + 4;
    // trip 1, the 32x32 pixels of the tile itself: a lane tests four adjacent pixels (row ry, columns rx .. rx + 3 of the
    // 34x34 grid) on the 7 x 3 dwords around them
    {
        const int ry = 1 + (tid >> 3), g = tid & 7, rx = 1 + 4 * g;
        u32 w[7][3];
#pragma unroll
        for (int r = 0; r < 7; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q) w[r][q] = s_img4[(ry + r) * FT_P + g + q];
        const FastQuad Q(w);
        if (__any(Q.candidate())) {
            u32 mb[2], md[2];
            Q.masks(mb, md);
            const int gy = y0 + ry - 1;
            const bool row_in = gy >= 3 && gy < L.h - 3;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const u32 sel = (k & 2) ? 0x03020302u : 0x01000100u;
                const bool br = fast_run9(__builtin_amdgcn_perm(mb[k & 1], mb[k & 1], sel));
                const bool dk = fast_run9(__builtin_amdgcn_perm(md[k & 1], md[k & 1], sel));
                const int gx = x0 + rx - 1 + k;
                if ((br || dk) && row_in && gx >= 3 && gx < L.w - 3)
                    s_corner[atomicAdd(&s_nc, 1)] = (unsigned short)((ry << 6) | (rx + k) | (br ? 0 : 0x8000));
            }
        }
    }
    // trip 2, the 132 pixels of the ring around the tile, one per lane
    {
        const int i = tid;
        const int ry = i < FT + 2 ? 0 : (i < 2 * (FT + 2) ? FT + 1 : (i < 3 * FT + 4 ? i - (2 * FT + 3) : i - (3 * FT + 3)));
        const int rx = i < FT + 2 ? i : (i < 2 * (FT + 2) ? i - (FT + 2) : (i < 3 * FT + 4 ? 0 : FT + 1));
        const int gy = y0 + ry - 1, gx = x0 + rx - 1;
        int pol = 0;
        bool cand = false;
        const uint8_t *pc = s_img + (ry + 3) * IS + (rx + 3);
        const bool inside = i < 4 * FT + 4 && gx >= 3 && gx < L.w - 3 && gy >= 3 && gy < L.h - 3;
        if (inside) {
            const int c = pc[0];
            const int v0 = (int)pc[3 * IS] - c, v4 = (int)pc[3] - c, v8 = (int)pc[-3 * IS] - c, v12 = (int)pc[-3] - c;
            const int nb = (v0 > RELOC_FAST_THRESHOLD) + (v4 > RELOC_FAST_THRESHOLD) + (v8 > RELOC_FAST_THRESHOLD) + (v12 > RELOC_FAST_THRESHOLD);
            const int nd = (v0 < -RELOC_FAST_THRESHOLD) + (v4 < -RELOC_FAST_THRESHOLD) + (v8 < -RELOC_FAST_THRESHOLD) + (v12 < -RELOC_FAST_THRESHOLD);
            cand = nb >= 2 || nd >= 2;
        }
        if (tid < 3 * 64 && __any(cand)) {
            if (cand) pol = fast_is_corner(pc, IS, RELOC_FAST_THRESHOLD);
        }
        if (pol) s_corner[atomicAdd(&s_nc, 1)] = (unsigned short)((ry << 6) | rx | (pol < 0 ? 0x8000 : 0));
    }
    __syncthreads();
    for (int i = tid; i < s_nc; i += 256) {
        const int e16 = s_corner[i], ry = (e16 >> 6) & 63, rx = e16 & 63;
        s_sc[ry * SS + rx] = (uint8_t)fast_corner_score(s_img + (ry + 3) * IS + (rx + 3), IS, RELOC_FAST_THRESHOLD, (e16 & 0x8000) ? -1 : 1);
    }
    __syncthreads();
    {
        const int ry = tid / 8, rx4 = (tid % 8) * 4;
        u32 word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int gx = x0 + rx4 + k, gy = y0 + ry;
            const uint8_t *s = s_sc + (ry + 1) * SS + (rx4 + k + 1);
            const int c = s[0];
            if (c && gx >= e && gx < L.w - e && gy >= e && gy < L.h - e && c > s[-1] && c > s[1] && c > s[-SS - 1] &&
                c > s[-SS] && c > s[-SS + 1] && c > s[SS - 1] && c > s[SS] && c > s[SS + 1]) {
                word |= (u32)c << (8 * k);
                atomicAdd(&s_hist[c], 1);
            }
        }
        const int gy = y0 + ry;
        if (gy < L.h) *reinterpret_cast<u32 *>(out + (size_t)gy * L.stride + x0 + rx4) = word;
    }
    __syncthreads();
    if (s_hist[tid]) atomicAdd(&hist[l * 256 + tid], s_hist[tid]);
}

// ---- stage 1 cut + Harris -----------------------------------------------------------------------
__device__ float harris_px(const uint8_t *p, int step)
{
    int a = 0, b = 0, c = 0;
#pragma unroll
    for (int dy = -3; dy <= 3; ++dy)
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const uint8_t *q = p + dy * step + dx;
            const int ix = (q[1] - q[-1]) * 2 + (q[-step + 1] - q[-step - 1]) + (q[step + 1] - q[step - 1]);
            const int iy = (q[step] - q[-step]) * 2 + (q[step - 1] - q[-step - 1]) + (q[step + 1] - q[-step + 1]);
            a += ix * ix;
            b += iy * iy;
            c += ix * iy;
        }
    const float scale = __fdiv_rn(1.f, (float)((1 << 2) * RELOC_HARRIS_BLOCK) * 255.f);
    const float s2 = __fmul_rn(scale, scale), s3 = __fmul_rn(s2, scale), s4 = __fmul_rn(s3, scale);
    const float fa = (float)a, fb = (float)b, fc = (float)c;
    const float t1 = __fmul_rn(fa, fb), t2 = __fmul_rn(fc, fc), t3 = __fadd_rn(fa, fb);
    const float t4 = __fmul_rn(RELOC_HARRIS_K, t3), t5 = __fmul_rn(t4, t3);
    const float t6 = __fsub_rn(t1, t2), t7 = __fsub_rn(t6, t5);
    return __fmul_rn(t7, s4);
}

// FAST + NMS tiles and 7x7 blur tiles of all levels in ONE launch, one workgroup per tile: both only read the pyramid, FAST
// feeds Harris and the blur feeds the descriptors, so they need not run one after the other.  (A smaller grid whose workgroups
// walk the tiles paid beside 112-register scans and pays nothing beside 104-register ones: profiles/README.md "Dropped
// experiments" #8.)
__global__ __launch_bounds__(256) void k_fast_blur(const OrbTable *__restrict__ tab, const uint8_t *__restrict__ pyr,
                                                   uint8_t *__restrict__ nms, int32_t *__restrict__ hist,
                                                   uint8_t *__restrict__ blur, int n_fast)
{
    RELOC_SMALL_KERNEL_PRIO();
    if ((int)blockIdx.x < n_fast) fast_nms_tile(tab, pyr, nms, hist, (int)blockIdx.x);
    else blur7_tile(tab, pyr, blur, (int)blockIdx.x - n_fast);
}
__global__ __launch_bounds__(256) void k_fast_blur_batch(OrbBatch b, int n_fast)
{
    RELOC_SMALL_KERNEL_PRIO();
    const OrbFrame &F = b.f[blockIdx.y];
    if ((int)blockIdx.x < n_fast) fast_nms_tile(F.tab, F.pyr, F.nms, F.hist, (int)blockIdx.x);
    else blur7_tile(F.tab, F.pyr, F.blur, (int)blockIdx.x - n_fast);
}


// cut score from the level's histogram (KeyPointsFilter::retainBest(2*quota) with ties kept, raised
// while the kept set exceeds RELOC_ORB_STAGE1_CAP), by ONE wave without block barriers: lane i owns the
// bins 4i .. 4i+3.  c(s) = sum_{k >= s} hist[k] is non-increasing in s;
//   cut0 = max{s : c(s) >= n_keep} if c(0) > n_keep, else the FAST threshold (everything is kept);
//   cut  = min{s >= cut0 : c(s) <= CAP or s == 255}.
// Every lane returns the cut.
__device__ int stage1_cut_wave(const int32_t *__restrict__ hist_l, int n_keep, int lane)
{
    const int4 h = *reinterpret_cast<const int4 *>(hist_l + 4 * lane);
    // exclusive suffix sum of the lane totals
    const int mine = h.x + h.y + h.z + h.w;
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_down(incl, d);
        if (lane + d < 64) incl += v;
    }
    const int above = incl - mine;
    const int c3 = h.w + above, c2 = h.z + c3, c1 = h.y + c2, c0 = h.x + c1;     // c(4i+3) .. c(4i)
    const int total = __builtin_amdgcn_readlane(c0, 0);
    int cut0 = RELOC_FAST_THRESHOLD;
    if (total > n_keep) {
        const int s = c3 >= n_keep ? 3 : (c2 >= n_keep ? 2 : (c1 >= n_keep ? 1 : (c0 >= n_keep ? 0 : -1)));
        cut0 = (int)wave_max_u32(s < 0 ? 0u : (unsigned)(4 * lane + s + 1)) - 1;
    }
    // smallest s >= cut0 with c(s) <= CAP (or 255): largest of 256 - s over the admissible bins
    unsigned best = 0;
    const int cs[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        const int s = 4 * lane + k;
        if (s >= cut0 && (cs[k] <= RELOC_ORB_STAGE1_CAP || s == 255)) best = (unsigned)(256 - s);
    }
    return 256 - (int)wave_max_u32(best);
}

// Harris response of one pixel by a whole wave: lanes 0..48 own one pixel of the 7x7 block each.
// harris_terms: the lane's three products (its byte loads); harris_finish: wave sums + the float formula.
__device__ __forceinline__ void harris_terms(const uint8_t *p, int step, int lane, int &a, int &b, int &c)
{
    a = b = c = 0;
    if (lane < 49) {
        const int dy = lane / 7 - 3, dx = lane % 7 - 3;
        const uint8_t *q = p + dy * step + dx;
        const int ix = (q[1] - q[-1]) * 2 + (q[-step + 1] - q[-step - 1]) + (q[step + 1] - q[step - 1]);
        const int iy = (q[step] - q[-step]) * 2 + (q[step - 1] - q[-step - 1]) + (q[step + 1] - q[-step + 1]);
        a = ix * ix; b = iy * iy; c = ix * iy;
    }
}

__device__ __forceinline__ float harris_finish(int a, int b, int c)
{
    a = wave_sum_i32(a);                  // integer sums: exact in any order
    b = wave_sum_i32(b);
    c = wave_sum_i32(c);
    const float scale = __fdiv_rn(1.f, (float)((1 << 2) * RELOC_HARRIS_BLOCK) * 255.f);
    const float s2 = __fmul_rn(scale, scale), s3 = __fmul_rn(s2, scale), s4 = __fmul_rn(s3, scale);
    const float fa = (float)a, fb = (float)b, fc = (float)c;
    const float t1 = __fmul_rn(fa, fb), t2 = __fmul_rn(fc, fc), t3 = __fadd_rn(fa, fb);
    const float t4 = __fmul_rn(RELOC_HARRIS_K, t3), t5 = __fmul_rn(t4, t3);
    const float t6 = __fsub_rn(t1, t2), t7 = __fsub_rn(t6, t5);
    return __fmul_rn(t7, s4);
}

// Each block scans HARRIS_CHUNK bytes of the NMS map, collects the survivors >= cut in LDS, then its four waves
// compute their Harris responses (one wave per survivor) and append them to the level's candidate list.
// Corners cluster, and a block works through its survivors four at a time: small chunks keep the longest
// block short (ORB stage 77.5 us with 4096-byte chunks, 75.7 us with 1024-byte chunks).
__device__ __forceinline__ void harris_body(const OrbTable *__restrict__ tab, const uint8_t *__restrict__ pyr,
                                                const uint8_t *__restrict__ nms, const int32_t *__restrict__ hist,
                                                int32_t *__restrict__ cand_cnt, u32 *__restrict__ cand_key,
                                                float *__restrict__ cand_resp, int32_t *__restrict__ dbg_cut)
{
    __shared__ int s_cut;
    __shared__ int s_n, s_base;
    __shared__ u32 s_list[HARRIS_CHUNK];
    const int l = find_level(tab->flat_base, blockIdx.x);
    const OrbLevel L = tab->lev[l];
    if (L.quota <= 0 || L.w <= 2 * RELOC_ORB_EDGE || L.h <= 2 * RELOC_ORB_EDGE) return;
    const int64_t idx0 = ((int64_t)(blockIdx.x - tab->flat_base[l]) * 256 + threadIdx.x) * (HARRIS_CHUNK / 256);
    const int64_t total = (int64_t)L.stride * L.h;
    u32 v = 0;
    if (idx0 < total) v = *reinterpret_cast<const u32 *>(nms + L.off + idx0);
    const bool any = v != 0;
    if (threadIdx.x == 0) s_n = 0;
    if (!__syncthreads_or(any)) return;                      // nothing kept in this chunk: skip the cut computation
    if (threadIdx.x < 64) {
        const int c = stage1_cut_wave(hist + l * 256, 2 * L.quota, threadIdx.x);
        if (threadIdx.x == 0) {
            s_cut = c;
            if (dbg_cut) dbg_cut[l] = c;
        }
    }
    __syncthreads();
    const int cut = s_cut;
    if (any) {
#pragma unroll
        for (int k = 0; k < HARRIS_CHUNK / 256; ++k) {
            const int sc = (v >> (8 * k)) & 0xFF;
            if (sc && sc >= cut) {
                const int64_t idx = idx0 + k;
                const int y = (int)(idx / L.stride), x = (int)(idx % L.stride);
                s_list[atomicAdd(&s_n, 1)] = ((u32)y << 16) | (u32)x;
            }
        }
    }
    __syncthreads();
    const int n = s_n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *img = pyr + L.off;
    // ONE slot reservation per block, its round trip hidden behind the first responses (the per-survivor atomicAdd it
    // replaces was a second memory round trip in every turn); each wave takes two survivors per turn so that the pixel
    // loads of the second are in flight while the first is reduced.
    int base_ret = 0;
    if (threadIdx.x == 0 && n > 0) base_ret = atomicAdd(&cand_cnt[l], n);
    auto terms = [&](u32 key, int &a, int &b, int &c) {
        harris_terms(img + (size_t)(key >> 16) * L.stride + (key & 0xFFFF), L.stride, lane, a, b, c);
    };
    int i = wave * 2;
    const bool first = i < n;                                  // wave-uniform
    u32 k0 = 0, k1 = 0;
    int a0 = 0, b0 = 0, c0 = 0, a1 = 0, b1 = 0, c1 = 0;
    float h0 = 0.f, h1 = 0.f;
    if (first) {
        k0 = s_list[i]; k1 = s_list[i + 1 < n ? i + 1 : i];
        terms(k0, a0, b0, c0);
        terms(k1, a1, b1, c1);
    }
    if (threadIdx.x == 0) s_base = base_ret;
    if (first) { h0 = harris_finish(a0, b0, c0); h1 = harris_finish(a1, b1, c1); }
    __syncthreads();
    const int base = s_base;
    auto put = [&](int at, u32 key, float r) {
        const int pos = base + at;
        if (pos < RELOC_ORB_STAGE1_CAP) {
            cand_key[(size_t)l * RELOC_ORB_STAGE1_CAP + pos] = key;
            cand_resp[(size_t)l * RELOC_ORB_STAGE1_CAP + pos] = r;
        }
    };
    if (first && lane == 0) {
        put(i, k0, h0);
        if (i + 1 < n) put(i + 1, k1, h1);
    }
    for (i += 8; i < n; i += 8) {
        k0 = s_list[i]; k1 = s_list[i + 1 < n ? i + 1 : i];
        terms(k0, a0, b0, c0);
        terms(k1, a1, b1, c1);
        h0 = harris_finish(a0, b0, c0);
        h1 = harris_finish(a1, b1, c1);
        if (lane == 0) {
            put(i, k0, h0);
            if (i + 1 < n) put(i + 1, k1, h1);
        }
    }
}
__global__ __launch_bounds__(256) void k_harris(const OrbTable *__restrict__ tab, const uint8_t *__restrict__ pyr,
                                                const uint8_t *__restrict__ nms, const int32_t *__restrict__ hist,
                                                int32_t *__restrict__ cand_cnt, u32 *__restrict__ cand_key,
                                                float *__restrict__ cand_resp, int32_t *__restrict__ dbg_cut)
{
    RELOC_SMALL_KERNEL_PRIO();
    harris_body(tab, pyr, nms, hist, cand_cnt, cand_key, cand_resp, dbg_cut);
}
__global__ __launch_bounds__(256) void k_harris_batch(OrbBatch b)
{
    RELOC_SMALL_KERNEL_PRIO();
    const OrbFrame &F = b.f[blockIdx.y];
    harris_body(F.tab, F.pyr, F.nms, F.hist, F.cand_cnt, F.cand_key, F.cand_resp, F.dbg_cut);
}


// ---- stage 2: best quota by Harris (ties kept), raster order -----------------------------------
// One workgroup per level.  Element i is kept iff fewer than `quota` responses are strictly greater
// (= best quota plus every tie of the quota-th); the kept ones are then placed in raster order by
// counting smaller keys.  Quadratic in the list length, which is ~2*quota (a few hundred).
__device__ __forceinline__ void select_body(const OrbTable *__restrict__ tab, const int32_t *__restrict__ cand_cnt,
                                                 const u32 *__restrict__ cand_key, const float *__restrict__ cand_resp,
                                                 int32_t *__restrict__ kp_cnt, u32 *__restrict__ kp_key,
                                                 float *__restrict__ kp_resp)
{
    __shared__ u32 s_key[RELOC_ORB_STAGE1_CAP];
    __shared__ float s_resp[RELOC_ORB_STAGE1_CAP];
    __shared__ u32 s_kidx[RELOC_ORB_STAGE1_CAP];
    __shared__ int s_nk;
    const int l = blockIdx.x;
    const int quota = tab->lev[l].quota;
    const int M = min(cand_cnt[l], RELOC_ORB_STAGE1_CAP);
    const int tid = threadIdx.x;
    if (tid == 0) s_nk = 0;
    for (int i = tid; i < M; i += 1024) {
        s_key[i] = cand_key[(size_t)l * RELOC_ORB_STAGE1_CAP + i];
        s_resp[i] = cand_resp[(size_t)l * RELOC_ORB_STAGE1_CAP + i];
    }
    __syncthreads();
    for (int i = tid; i < M; i += 1024) {
        const float r = s_resp[i];
        int greater = 0;
        for (int j = 0; j < M; ++j) greater += s_resp[j] > r;
        if (greater < quota) s_kidx[atomicAdd(&s_nk, 1)] = (u32)i;
    }
    __syncthreads();
    const int K = s_nk;
    for (int i = tid; i < K; i += 1024) {
        const u32 src = s_kidx[i];
        const u32 key = s_key[src];
        int pos = 0;
        for (int j = 0; j < K; ++j) pos += s_key[s_kidx[j]] < key;
        kp_key[(size_t)l * RELOC_ORB_STAGE1_CAP + pos] = key;
        kp_resp[(size_t)l * RELOC_ORB_STAGE1_CAP + pos] = s_resp[src];
    }
    if (tid == 0) kp_cnt[l] = K;
}
__global__ __launch_bounds__(1024) void k_select(const OrbTable *__restrict__ tab, const int32_t *__restrict__ cand_cnt,
                                                 const u32 *__restrict__ cand_key, const float *__restrict__ cand_resp,
                                                 int32_t *__restrict__ kp_cnt, u32 *__restrict__ kp_key,
                                                 float *__restrict__ kp_resp)
{
    RELOC_SMALL_KERNEL_PRIO();
    select_body(tab, cand_cnt, cand_key, cand_resp, kp_cnt, kp_key, kp_resp);
}
__global__ __launch_bounds__(1024) void k_select_batch(OrbBatch b)
{
    RELOC_SMALL_KERNEL_PRIO();
    const OrbFrame &F = b.f[blockIdx.y];
    select_body(F.tab, F.cand_cnt, F.cand_key, F.cand_resp, F.kp_cnt, F.kp_key, F.kp_resp);
}


// ---- orientation + descriptor -------------------------------------------------------------------
__device__ float fast_atan2_deg(float y, float x)
{
    const float ax = fabsf(x), ay = fabsf(y);
    float a;
    if (ax >= ay) {
        const float c = __fdiv_rn(ay, __fadd_rn(ax, RELOC_ATAN2_EPS));
        const float c2 = __fmul_rn(c, c);
        float t = __fadd_rn(__fmul_rn(RELOC_ATAN2_P7, c2), RELOC_ATAN2_P5);
        t = __fadd_rn(__fmul_rn(t, c2), RELOC_ATAN2_P3);
        t = __fadd_rn(__fmul_rn(t, c2), RELOC_ATAN2_P1);
        a = __fmul_rn(t, c);
    } else {
        const float c = __fdiv_rn(ax, __fadd_rn(ay, RELOC_ATAN2_EPS));
        const float c2 = __fmul_rn(c, c);
        float t = __fadd_rn(__fmul_rn(RELOC_ATAN2_P7, c2), RELOC_ATAN2_P5);
        t = __fadd_rn(__fmul_rn(t, c2), RELOC_ATAN2_P3);
        t = __fadd_rn(__fmul_rn(t, c2), RELOC_ATAN2_P1);
        t = __fmul_rn(t, c);
        a = __fsub_rn(90.f, t);
    }
    if (x < 0) a = __fsub_rn(180.f, a);
    if (y < 0) a = __fsub_rn(360.f, a);
    return a;
}

__device__ void sincos_spec(double th, float *s_out, float *c_out)
{
    const double PIO2_HI = 1.57079632679489655800e+00;
    const double PIO2_LO = 6.12323399573676603587e-17;
    const double TWO_OVER_PI = 6.36619772367581382433e-01;
    const double kd = floor(__dadd_rn(__dmul_rn(th, TWO_OVER_PI), 0.5));
    const int k = (int)kd;
    double r = __dsub_rn(th, __dmul_rn(kd, PIO2_HI));
    r = __dsub_rn(r, __dmul_rn(kd, PIO2_LO));
    const double r2 = __dmul_rn(r, r);
    const double S[8] = {-1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0,
                         1.0 / 6227020800.0, -1.0 / 1307674368000.0, 1.0 / 355687428096000.0};
    const double C[8] = {-1.0 / 2.0, 1.0 / 24.0, -1.0 / 720.0, 1.0 / 40320.0, -1.0 / 3628800.0,
                         1.0 / 479001600.0, -1.0 / 87178291200.0, 1.0 / 20922789888000.0};
    double ps = S[7], pc = C[7];
#pragma unroll
    for (int i = 6; i >= 0; --i) {
        ps = __dadd_rn(__dmul_rn(ps, r2), S[i]);
        pc = __dadd_rn(__dmul_rn(pc, r2), C[i]);
    }
    ps = __dmul_rn(__dadd_rn(__dmul_rn(ps, r2), 1.0), r);
    pc = __dadd_rn(__dmul_rn(pc, r2), 1.0);
    double sn, cs;
    switch (k & 3) {
    case 0: sn = ps; cs = pc; break;
    case 1: sn = pc; cs = -ps; break;
    case 2: sn = -ps; cs = -pc; break;
    default: sn = -pc; cs = ps; break;
    }
    *s_out = (float)sn;
    *c_out = (float)cs;
}

// one wave per keypoint; block = 4 waves
__device__ __forceinline__ void describe_body(const OrbTable *__restrict__ tab, const uint8_t *__restrict__ pyr,
                                                  const uint8_t *__restrict__ blur, const int32_t *__restrict__ kp_cnt,
                                                  const u32 *__restrict__ kp_key, const float *__restrict__ kp_resp,
                                                  int max_feat, float *__restrict__ f_xy, float *__restrict__ f_size,
                                                  float *__restrict__ f_angle, float *__restrict__ f_resp,
                                                  int32_t *__restrict__ f_oct, uint8_t *__restrict__ f_desc,
                                                  int32_t *__restrict__ f_count)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    int base[NLEV + 1];
    base[0] = 0;
#pragma unroll
    for (int l = 0; l < NLEV; ++l) base[l + 1] = base[l] + kp_cnt[l];
    const int total = base[NLEV];
    if (g == 0 && lane == 0) *f_count = min(total, max_feat);
    if (g >= total || g >= max_feat) return;
    int l = 0;
#pragma unroll
    for (int k = 1; k < NLEV; ++k) l += g >= base[k];
    const OrbLevel L = tab->lev[l];
    const int i = g - base[l];
    const u32 key = kp_key[(size_t)l * RELOC_ORB_STAGE1_CAP + i];
    const int x = key & 0xFFFF, y = key >> 16;
    const uint8_t *center = pyr + L.off + (size_t)y * L.stride + x;
    // intensity-centroid moments: 31 rows, lane = column offset (-15..15 -> lanes 0..30), two rows at a time
    int m10 = 0, m01 = 0;
    {
        const int u = (lane & 31) - 15;            // -15..16 (16 unused)
        const int half = lane >> 5;                // rows split between the two half-waves
        for (int vv = half; vv <= 30; vv += 2) {
            const int v = vv - 15;
            const int av = v < 0 ? -v : v;
            if (u <= 15 && (u < 0 ? -u : u) <= c_umax[av]) {
                const int I = center[v * L.stride + u];
                m10 += u * I;
                m01 += v * I;
            }
        }
        m10 = wave_sum_i32(m10);
        m01 = wave_sum_i32(m01);
    }
    const float angle = fast_atan2_deg((float)m01, (float)m10);
    float sn, cs;
    sincos_spec((double)__fmul_rn(angle, RELOC_DEG2RAD_F), &sn, &cs);
    const uint8_t *bc = blur + L.off + (size_t)y * L.stride + x;
    unsigned long long bits[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const signed char *t = c_pattern + 4 * (64 * it + lane);
        int val[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float px = (float)t[2 * e], py = (float)t[2 * e + 1];
            const float rx = __fsub_rn(__fmul_rn(px, cs), __fmul_rn(py, sn));
            const float ry = __fadd_rn(__fmul_rn(px, sn), __fmul_rn(py, cs));
            const int ix = (int)rintf(rx), iy = (int)rintf(ry);
            val[e] = bc[iy * L.stride + ix];
        }
        bits[it] = __ballot(val[0] < val[1]);
    }
    if (lane < 4) {
        const unsigned long long b = lane == 0 ? bits[0] : lane == 1 ? bits[1] : lane == 2 ? bits[2] : bits[3];
        reinterpret_cast<unsigned long long *>(f_desc + (size_t)g * 32)[lane] = b;
    }
    if (lane == 0) {
        f_xy[2 * g] = __fmul_rn((float)x, L.scale);
        f_xy[2 * g + 1] = __fmul_rn((float)y, L.scale);
        f_size[g] = __fmul_rn((float)RELOC_ORB_PATCH, L.scale);
        f_angle[g] = angle;
        f_resp[g] = kp_resp[(size_t)l * RELOC_ORB_STAGE1_CAP + i];
        f_oct[g] = l;
    }
}
__global__ __launch_bounds__(256) void k_describe(const OrbTable *__restrict__ tab, const uint8_t *__restrict__ pyr,
                                                  const uint8_t *__restrict__ blur, const int32_t *__restrict__ kp_cnt,
                                                  const u32 *__restrict__ kp_key, const float *__restrict__ kp_resp,
                                                  int max_feat, float *__restrict__ f_xy, float *__restrict__ f_size,
                                                  float *__restrict__ f_angle, float *__restrict__ f_resp,
                                                  int32_t *__restrict__ f_oct, uint8_t *__restrict__ f_desc,
                                                  int32_t *__restrict__ f_count)
{
    RELOC_SMALL_KERNEL_PRIO();
    describe_body(tab, pyr, blur, kp_cnt, kp_key, kp_resp, max_feat, f_xy, f_size, f_angle, f_resp, f_oct, f_desc, f_count);
}
__global__ __launch_bounds__(256) void k_describe_batch(OrbBatch b, int max_feat)
{
    RELOC_SMALL_KERNEL_PRIO();
    const OrbFrame &F = b.f[blockIdx.y];
    describe_body(F.tab, F.pyr, F.blur, F.kp_cnt, F.kp_key, F.kp_resp, max_feat, F.f_xy, F.f_size, F.f_angle, F.f_resp, F.f_oct, F.f_desc,
                  F.f_count);
}


// ------------------------------------------------------------------------------------------------
static void resize_axis(int src_n, int dst_n, int32_t *ofs, int32_t *coef)
{
    const double scale = (double)src_n / (double)dst_n;
    for (int d = 0; d < dst_n; ++d) {
        double f = ((double)d + 0.5) * scale - 0.5;
        int s = (int)floor(f);
        double a = f - (double)s;
        if (s < 0) { s = 0; a = 0.0; }
        if (s >= src_n - 1) { s = src_n - 1; a = 0.0; }
        ofs[d] = s;
        coef[d] = (int32_t)lrint(a * (double)(1 << RELOC_RESIZE_COEF_BITS));
    }
}

static bool g_pattern_uploaded[64] = {};

int orb_prepare(reloc_ctx *ctx, int w, int h, int nfeatures)
{
    if (w > ctx->max_w || h > ctx->max_h) {
        reloc_set_error("frame %dx%d exceeds the ctx capacity %dx%d", w, h, ctx->max_w, ctx->max_h);
        return RELOC_E_CAPACITY;
    }
    if (ctx->orb_w == w && ctx->orb_h == h && ctx->orb_nfeat == nfeatures) return RELOC_OK;
    if (!g_pattern_uploaded[ctx->device & 63]) {
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_pattern), RELOC_ORB_PATTERN, sizeof(RELOC_ORB_PATTERN)));
        g_pattern_uploaded[ctx->device & 63] = true;
    }
    OrbTable tab;
    memset(&tab, 0, sizeof(tab));
    int64_t off = 0;
    for (int l = 0; l < NLEV; ++l) {
        const float s = (float)pow(RELOC_ORB_SCALE_FACTOR, (double)l);
        OrbLevel &L = tab.lev[l];
        L.scale = s;
        L.w = (int)lrintf((float)w / s);
        L.h = (int)lrintf((float)h / s);
        L.stride = (L.w + 63) / 64 * 64;
        L.off = off;
        off += ((int64_t)L.stride * L.h + 255) / 256 * 256;
    }
    if (off > ctx->pyr_bytes) { reloc_set_error("pyramid arena too small"); return RELOC_E_CAPACITY; }
    {
        const float factor = (float)(1.0 / RELOC_ORB_SCALE_FACTOR);
        float nper = (float)(nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)NLEV)));
        int sum = 0;
        for (int l = 0; l < NLEV - 1; ++l) {
            tab.lev[l].quota = (int)lrintf(nper);
            sum += tab.lev[l].quota;
            nper *= factor;
        }
        tab.lev[NLEV - 1].quota = nfeatures - sum > 0 ? nfeatures - sum : 0;
    }
    for (int l = 0; l < NLEV; ++l) {
        const OrbLevel &L = tab.lev[l];
        tab.fast_tile_base[l + 1] = tab.fast_tile_base[l] + (L.stride / FT) * ((L.h + FT - 1) / FT);
        tab.blur_tile_base[l + 1] = tab.blur_tile_base[l] + ((L.w + BT_W - 1) / BT_W) * ((L.h + BT_H - 1) / BT_H);
        tab.flat_base[l + 1] = tab.flat_base[l] + (int)(((int64_t)L.stride * L.h + HARRIS_CHUNK - 1) / HARRIS_CHUNK);
    }
    // resize tables
    const int maxdim = ctx->max_w > ctx->max_h ? ctx->max_w : ctx->max_h;
    int32_t *host = (int32_t *)malloc(sizeof(int32_t) * (size_t)NLEV * 4 * maxdim);
    int pos = 0;
    for (int l = 1; l < NLEV; ++l) {
        const OrbLevel &S = tab.lev[l - 1], &D = tab.lev[l];
        tab.rz_off[l][0] = pos; tab.rz_off[l][1] = pos + D.w;
        resize_axis(S.w, D.w, host + pos, host + pos + D.w);
        pos += 2 * D.w;
        tab.rz_off[l][2] = pos; tab.rz_off[l][3] = pos + D.h;
        resize_axis(S.h, D.h, host + pos, host + pos + D.h);
        pos += 2 * D.h;
    }
    // fused-pyramid tiles: every tile owns a rectangle of every level (proportional split, x on 4-pixel
    // boundaries, the last column of tiles takes the row padding of levels >= 1, which is stored as 0)
    // and computes what the levels above need from it (k_pyramid).
    const int ntx = (w + PT_W - 1) / PT_W, nty = (h + PT_H - 1) / PT_H;
    PyrTile *tiles = (PyrTile *)calloc((size_t)ntx * nty, sizeof(PyrTile));
    int lds_lev[NLEV] = {}, lds_t = 0;
    for (int t = 0; t < ntx * nty; ++t) {
        const int tx = t % ntx, ty = t / ntx;
        PyrTile &T = tiles[t];
        int nx0 = 0, nx1 = 0, ny0 = 0, ny1 = 0;    // needed rectangle of the level above (empty)
        int tsum = 0;
        for (int l = NLEV - 1; l >= 0; --l) {
            const OrbLevel &L = tab.lev[l];
            const int quads = (l == 0 ? (L.w + 3) / 4 : L.stride / 4);
            const int ox0 = 4 * (int)((int64_t)tx * quads / ntx), ox1 = 4 * (int)((int64_t)(tx + 1) * quads / ntx);
            const int oy0 = (int)((int64_t)ty * L.h / nty), oy1 = (int)((int64_t)(ty + 1) * L.h / nty);
            T.o[l][0] = (uint16_t)ox0; T.o[l][1] = (uint16_t)ox1; T.o[l][2] = (uint16_t)oy0; T.o[l][3] = (uint16_t)oy1;
            // computed rectangle = own pixels (inside the image) united with the taps of the level above
            int cx0 = ox0, cx1 = ox1 < L.w ? ox1 : L.w, cy0 = oy0, cy1 = oy1;
            const bool stores = ox0 < ox1 && oy0 < oy1;                     // may be row padding only
            const bool own = cx0 < cx1 && cy0 < cy1, need = nx0 < nx1 && ny0 < ny1;
            if (need) {
                const int32_t *xo = host + tab.rz_off[l + 1][0], *yo = host + tab.rz_off[l + 1][2];
                int sx0 = xo[nx0], sx1 = xo[nx1 - 1] + 2, sy0 = yo[ny0], sy1 = yo[ny1 - 1] + 2;
                if (sx1 > L.w) sx1 = L.w;
                if (sy1 > L.h) sy1 = L.h;
                if (own) {
                    cx0 = cx0 < sx0 ? cx0 : sx0; cx1 = cx1 > sx1 ? cx1 : sx1;
                    cy0 = cy0 < sy0 ? cy0 : sy0; cy1 = cy1 > sy1 ? cy1 : sy1;
                } else {
                    cx0 = sx0; cx1 = sx1; cy0 = sy0; cy1 = sy1;
                }
            } else if (!own) {
                cx0 = cx1 = cy0 = cy1 = 0;
            }
            cx0 &= ~3;
            T.n[l][0] = (uint16_t)cx0; T.n[l][1] = (uint16_t)cx1; T.n[l][2] = (uint16_t)cy0; T.n[l][3] = (uint16_t)cy1;
            if (!stores) T.o[l][0] = T.o[l][1] = T.o[l][2] = T.o[l][3] = 0;
            nx0 = cx0; nx1 = cx1; ny0 = cy0; ny1 = cy1;
            const int bytes = ((cx1 - cx0 + 3) / 4 * 4) * (cy1 - cy0);
            lds_lev[l] = bytes > lds_lev[l] ? bytes : lds_lev[l];
            if (l >= 1) tsum += (cx1 - cx0) + (cy1 - cy0);
        }
        lds_t = tsum > lds_t ? tsum : lds_t;
    }
    ctx->pyr_ntiles = ntx * nty;
    {
        int o = 0;
        for (int l = 0; l < NLEV; ++l) { ctx->pyr_lds[l] = o; o += (lds_lev[l] + 15) / 16 * 16; }
        ctx->pyr_lds[NLEV] = o;
        ctx->pyr_lds_bytes = o + 4 * lds_t;
    }
    if (ctx->pyr_lds_bytes > 64 * 1024) { free(host); free(tiles); reloc_set_error("pyramid tile exceeds LDS"); return RELOC_E_CAPACITY; }
    hipError_t e0 = hipMemcpyAsync(ctx->pyr_tiles, tiles, sizeof(PyrTile) * (size_t)ntx * nty, hipMemcpyHostToDevice, ctx->stream);
    hipError_t e1 = hipMemcpyAsync(ctx->rz_tab, host, sizeof(int32_t) * (size_t)pos, hipMemcpyHostToDevice, ctx->stream);
    hipError_t e2 = hipMemcpyAsync(ctx->orb_const, &tab, sizeof(tab), hipMemcpyHostToDevice, ctx->stream);
    hipError_t e3 = hipStreamSynchronize(ctx->stream);
    free(host);
    free(tiles);
    HIP_TRY(e0); HIP_TRY(e1); HIP_TRY(e2); HIP_TRY(e3);
    memcpy(ctx->lev, tab.lev, sizeof(tab.lev));
    memcpy(ctx->orb_tab_host, &tab, sizeof(tab));
    ctx->orb_w = w; ctx->orb_h = h; ctx->orb_nfeat = nfeatures;
    return RELOC_OK;
}

// ---- CLAHE (include/reloc_spec.h) -------------------------------------------------------------------
// cv2.createCLAHE(clipLimit, tileGridSize).apply(gray) on 8-bit input, in two launches:
//   k_clahe_lut    one workgroup per tile: histogram of the tile's pixels of the padded frame (BORDER_REFLECT_101 on the
//                  right / bottom) in per-wave LDS sub-histograms (integer atomics: order-independent), then wave 0 holds
//                  4 bins per lane for the clip, the redistribution and the prefix sum and stores the tile's 256-byte LUT
//   k_clahe_apply  4 pixels per lane: gray (CH = 3: fused conversion), four LUT lookups through the cache, bilinear blend
// CH = 3 reads an interleaved frame (gray_fixed with the order / coefficient flags), CH = 1 a gray plane.  Both are
// frame-batched (blockIdx.y = frame); a single frame is a batch of one.
struct ClaheGeom {
    int w, h;              // frame size (the interpolation runs over it)
    int tx, ty;            // tile grid
    int tw, th;            // tile size in the padded frame
    int clip;              // clip count per bin, 0 = no clipping
    float lut_scale;       // 255.0f / (tw * th)
    float inv_tw, inv_th;  // 1.0f / tw, 1.0f / th
};
struct ClaheFrames { const uint8_t *src[RELOC_BATCH_MAX]; uint8_t *lut[RELOC_BATCH_MAX]; uint8_t *dst[RELOC_BATCH_MAX]; };
#ifndef RELOC_CLAHE_LUT_BS
#define RELOC_CLAHE_LUT_BS 1024
#endif
constexpr int CLAHE_LUT_BS = RELOC_CLAHE_LUT_BS;     // 16 waves, 16 sub-histograms (16 KB of LDS); see DESIGN.md for 256 / 512
constexpr int CLAHE_MAX_TILES = RELOC_CLAHE_MAX_TILES;

static ClaheGeom clahe_geom(int w, int h, double clip_limit, int tx, int ty)
{
    ClaheGeom g;
    g.w = w; g.h = h; g.tx = tx; g.ty = ty;
    // OpenCV pads BOTH axes unless both divide (a full extra tile on an axis that already divides)
    const bool divides = w % tx == 0 && h % ty == 0;
    g.tw = divides ? w / tx : (w + tx - w % tx) / tx;
    g.th = divides ? h / ty : (h + ty - h % ty) / ty;
    const int area = g.tw * g.th;
    if (clip_limit > 0.0) {
        const int c = (int)(clip_limit * area / 256);
        g.clip = c > 1 ? c : 1;
    } else {
        g.clip = 0;
    }
    g.lut_scale = 255.0f / (float)area;
    g.inv_tw = 1.0f / (float)g.tw;
    g.inv_th = 1.0f / (float)g.th;
    return g;
}

template <int CH>
__global__ __launch_bounds__(CLAHE_LUT_BS) void k_clahe_lut(ClaheFrames F, ClaheGeom g, int sstride, int flags)
{
    constexpr int NWAVE = CLAHE_LUT_BS / 64;
    __shared__ int s_hist[NWAVE][256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < NWAVE * 256; i += CLAHE_LUT_BS) (&s_hist[0][0])[i] = 0;
    __syncthreads();
    const uint8_t *src = F.src[blockIdx.y];
    const int ti = blockIdx.x % g.tx, tj = blockIdx.x / g.tx;
    const int x0 = ti * g.tw, y0 = tj * g.th;
    for (int py = wave; py < g.th; py += NWAVE) {
        const int sy = y0 + py < g.h ? y0 + py : reflect101(y0 + py, g.h);
        const uint8_t *row = src + (size_t)sy * sstride;
        for (int px = lane; px < g.tw; px += 64) {
            const int sx = x0 + px < g.w ? x0 + px : reflect101(x0 + px, g.w);
            int v;
            if (CH == 1) {
                v = row[sx];
            } else {
                const uint8_t *p = row + 3 * sx;
                const int c0 = p[0], c1 = p[1], c2 = p[2];
                v = gray_fixed((flags & 1) ? c2 : c0, c1, (flags & 1) ? c0 : c2, flags);
            }
            atomicAdd(&s_hist[wave][v], 1);
        }
    }
    __syncthreads();
    if (wave != 0) return;
    int hb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int s = 0;
#pragma unroll
        for (int wv = 0; wv < NWAVE; ++wv) s += s_hist[wv][4 * lane + k];
        hb[k] = s;
    }
    if (g.clip > 0) {
        int clipped = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ex = hb[k] > g.clip ? hb[k] - g.clip : 0;
            clipped += ex;
            hb[k] -= ex;
        }
        clipped = wave_sum_i32(clipped);
        const int batch = clipped >> 8, residual = clipped & 255;
        const int step = residual ? (256 / residual > 1 ? 256 / residual : 1) : 1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int bin = 4 * lane + k;
            hb[k] += batch + (residual && bin % step == 0 && bin / step < residual ? 1 : 0);
        }
    }
    // inclusive prefix sum: 4 bins in the lane, then the lanes' totals across the wave
    int loc[4];
    loc[0] = hb[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) loc[k] = loc[k - 1] + hb[k];
    int incl = loc[3];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    const int excl = incl - loc[3];
    u32 out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int v = __float2int_rn((float)(excl + loc[k]) * g.lut_scale);     // saturate_cast<uchar>: cvRound, then clamp
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        out |= (u32)v << (8 * k);
    }
    reinterpret_cast<u32 *>(F.lut[blockIdx.y] + (size_t)blockIdx.x * 256)[lane] = out;
}

template <int CH, bool ALIGNED>
__global__ __launch_bounds__(256) void k_clahe_apply(ClaheFrames F, ClaheGeom g, int sstride, int flags, int dstride)
{
    const int quads = (g.w + 3) >> 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= quads * g.h) return;
    const int y = q / quads, x4 = 4 * (q - y * quads);
    u32 d[3];
    pyr_fetch<CH, ALIGNED>(F.src[blockIdx.y] + (size_t)y * sstride + CH * x4, x4, g.w, d);
    const u32 gray4 = pyr_gray4<CH>(d, x4, g.w, flags);
    const float tyf = (float)y * g.inv_th - 0.5f;
    int ty1 = (int)floorf(tyf);
    const float ya = tyf - (float)ty1, ya1 = 1.0f - ya;
    const int ty2 = ty1 + 1 < g.ty - 1 ? ty1 + 1 : g.ty - 1;
    ty1 = ty1 > 0 ? ty1 : 0;
    const uint8_t *lut = F.lut[blockIdx.y];
    const uint8_t *L1 = lut + (size_t)ty1 * g.tx * 256, *L2 = lut + (size_t)ty2 * g.tx * 256;
    u32 out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x4 + k;
        const float txf = (float)x * g.inv_tw - 0.5f;
        int tx1 = (int)floorf(txf);
        const float xa = txf - (float)tx1, xa1 = 1.0f - xa;
        const int tx2 = tx1 + 1 < g.tx - 1 ? tx1 + 1 : g.tx - 1;
        tx1 = tx1 > 0 ? tx1 : 0;
        const int v = (gray4 >> (8 * k)) & 0xFF;
        const float l11 = L1[tx1 * 256 + v], l12 = L1[tx2 * 256 + v], l21 = L2[tx1 * 256 + v], l22 = L2[tx2 * 256 + v];
        const float res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya;
        int r = __float2int_rn(res);
        r = r < 0 ? 0 : (r > 255 ? 255 : r);
        if (x < g.w) out |= (u32)r << (8 * k);
    }
    uint8_t *dst = F.dst[blockIdx.y] + (size_t)y * dstride + x4;
    if ((dstride & 3) == 0) {
        *reinterpret_cast<u32 *>(dst) = out;       // the row holds round4(w) bytes: dstride >= w and a multiple of 4
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x4 + k < g.w) dst[k] = (uint8_t)(out >> (8 * k));
    }
}

// the two CLAHE launches for n frames of equal geometry on stream st; srcs: channels-interleaved rows of sstride bytes
static int clahe_launch(hipStream_t st, const ClaheFrames &F, int n, const ClaheGeom &g, int channels, int sstride, int flags,
                        int dstride)
{
    bool aligned = g.w % 4 == 0 && sstride % 4 == 0;
    for (int f = 0; f < n; ++f) aligned = aligned && ((uintptr_t)F.src[f]) % 4 == 0;
    const int quads = (g.w + 3) / 4;
    const dim3 glut(g.tx * g.ty, n), gapp((quads * g.h + 255) / 256, n);
    auto lut = channels == 3 ? k_clahe_lut<3> : k_clahe_lut<1>;
    auto app = channels == 3 ? (aligned ? k_clahe_apply<3, true> : k_clahe_apply<3, false>)
                             : (aligned ? k_clahe_apply<1, true> : k_clahe_apply<1, false>);
    hipLaunchKernelGGL(lut, glut, dim3(CLAHE_LUT_BS), 0, st, F, g, sstride, flags);
    hipLaunchKernelGGL(app, gapp, dim3(256), 0, st, F, g, sstride, flags, dstride);
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

static inline int clahe_stride(int w) { return (w + 63) & ~63; }

// ---- rectification: cv2.remap (include/reloc_spec.h, "REMAP") -----------------------------------------------
// OpenCV's fixed-point bilinear remap of 8-bit images through a map in the CV_16SC2 + CV_16UC1 form, BORDER_CONSTANT:
//   k_remap_u8<CH, GRAY>   4 output pixels per lane along x; the four taps of each pixel gathered through the cache (a
//                          rectification map is locally coherent: neighbouring lanes share lines).  CH = 3, GRAY: the
//                          stage in front of ORB -- gray of every tap on the fly (gray_fixed with the order / coefficient
//                          flags), then the blend, one dword store.  CH = 3 (3-channel output) and CH = 1 serve the shim.
//   k_remap_nearest<T, CH> the source pixel at xy (the fraction is ignored); T = uint16_t for the depth image
//   k_convert_maps         float maps -> the fixed-point form (cv2.convertMaps)
// All are frame-batched (blockIdx.y = frame) with per-frame map pointers; a single frame is a batch of one.
struct RemapFrames {
    const uint8_t *src[RELOC_BATCH_MAX]; const int16_t *xy[RELOC_BATCH_MAX]; const uint16_t *alpha[RELOC_BATCH_MAX];
    uint8_t *dst[RELOC_BATCH_MAX];
};
struct RemapGeom {
    int sw, sh, sstride;   // source size, row stride in bytes
    int dw, dh, dstride;   // map = destination size (maps are dense), destination row stride in bytes
    int border;            // BORDER_CONSTANT value
};

// one tap: the source pixel (x, y) or the border value; GRAY converts the 3 channels to one value
template <int CH, bool GRAY>
__device__ __forceinline__ void remap_tap(const uint8_t *__restrict__ src, const RemapGeom &g, int x, int y, int flags,
                                          int (&v)[GRAY ? 1 : CH])
{
    const bool in = (unsigned)x < (unsigned)g.sw && (unsigned)y < (unsigned)g.sh;
#pragma unroll
    for (int c = 0; c < (GRAY ? 1 : CH); ++c) v[c] = g.border;
    if (!in) return;
    const uint8_t *p = src + (size_t)y * g.sstride + CH * x;
    if (GRAY) {
        const int c0 = p[0], c1 = p[1], c2 = p[2];
        v[0] = gray_fixed((flags & 1) ? c2 : c0, c1, (flags & 1) ? c0 : c2, flags);
    } else {
#pragma unroll
        for (int c = 0; c < CH; ++c) v[c] = p[c];
    }
}

template <int CH, bool GRAY, bool ALIGNED>
__global__ __launch_bounds__(256) void k_remap_u8(RemapFrames F, RemapGeom g, int flags)
{
    constexpr int OC = GRAY ? 1 : CH;       // output channels
    const int quads = (g.dw + 3) >> 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= quads * g.dh) return;
    const int y = q / quads, x4 = 4 * (q - y * quads);
    const size_t m = (size_t)y * g.dw + x4;
    const int16_t *xyp = F.xy[blockIdx.y] + 2 * m;
    const uint16_t *ap = F.alpha[blockIdx.y] + m;
    u32 xy[4], al[4];
    if (ALIGNED) {      // dw % 4 == 0 and 16-byte aligned maps: 16 B of xy and 8 B of alpha per lane
        const uint4 a = *reinterpret_cast<const uint4 *>(xyp);
        const uint2 b = *reinterpret_cast<const uint2 *>(ap);
        xy[0] = a.x; xy[1] = a.y; xy[2] = a.z; xy[3] = a.w;
        al[0] = b.x & 0xFFFF; al[1] = b.x >> 16; al[2] = b.y & 0xFFFF; al[3] = b.y >> 16;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = x4 + k < g.dw;
            xy[k] = ok ? reinterpret_cast<const u32 *>(xyp)[k] : 0;
            al[k] = ok ? ap[k] : 0;
        }
    }
    const uint8_t *src = F.src[blockIdx.y];
    int out[4][OC];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int sx = (int16_t)(xy[k] & 0xFFFF), sy = (int16_t)(xy[k] >> 16);
        const int fx = al[k] & 31, fy = (al[k] >> 5) & 31;
        int p00[OC], p01[OC], p10[OC], p11[OC];
        remap_tap<CH, GRAY>(src, g, sx, sy, flags, p00);
        remap_tap<CH, GRAY>(src, g, sx + 1, sy, flags, p01);
        remap_tap<CH, GRAY>(src, g, sx, sy + 1, flags, p10);
        remap_tap<CH, GRAY>(src, g, sx + 1, sy + 1, flags, p11);
        const int w00 = 32 * (32 - fx) * (32 - fy), w01 = 32 * fx * (32 - fy), w10 = 32 * (32 - fx) * fy, w11 = 32 * fx * fy;
#pragma unroll
        for (int c = 0; c < OC; ++c) out[k][c] = (p00[c] * w00 + p01[c] * w01 + p10[c] * w10 + p11[c] * w11 + (1 << 14)) >> 15;
    }
    uint8_t *dst = F.dst[blockIdx.y] + (size_t)y * g.dstride + OC * x4;
    if (OC == 1 && (g.dstride & 3) == 0) {
        // the row holds round4(dw) bytes: dstride >= dw and a multiple of 4
        *reinterpret_cast<u32 *>(dst) = (u32)out[0][0] | (u32)out[1][0] << 8 | (u32)out[2][0] << 16 | (u32)out[3][0] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x4 + k < g.dw) {
#pragma unroll
                for (int c = 0; c < OC; ++c) dst[OC * k + c] = (uint8_t)out[k][c];
            }
    }
}

// nearest: one output pixel per lane; strides of src and dst in elements of T
template <typename T, int CH>
__global__ __launch_bounds__(256) void k_remap_nearest(RemapFrames F, RemapGeom g)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.z;
    if (x >= g.dw) return;
    const u32 xy = reinterpret_cast<const u32 *>(F.xy[blockIdx.y])[(size_t)y * g.dw + x];
    const int sx = (int16_t)(xy & 0xFFFF), sy = (int16_t)(xy >> 16);
    const bool in = (unsigned)sx < (unsigned)g.sw && (unsigned)sy < (unsigned)g.sh;
    const T *s = reinterpret_cast<const T *>(F.src[blockIdx.y]) + (size_t)(in ? sy : 0) * g.sstride + CH * (in ? sx : 0);
    T *d = reinterpret_cast<T *>(F.dst[blockIdx.y]) + (size_t)y * g.dstride + CH * x;
#pragma unroll
    for (int c = 0; c < CH; ++c) d[c] = in ? s[c] : (T)g.border;
}

// cvRound of an f32 to int32: half to even, saturating; NaN -> INT32_MIN (both far outside every image)
__device__ __forceinline__ int remap_round(float v)
{
    if (v != v) return INT32_MIN;
    const float r = rintf(v);
    if (r >= 2147483648.0f) return INT32_MAX;
    if (r <= -2147483648.0f) return INT32_MIN;
    return (int)r;
}
__device__ __forceinline__ int remap_sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// cv2.convertMaps(mapx, mapy, CV_16SC2, nninterpolation = nn): one map entry per lane
__global__ __launch_bounds__(256) void k_convert_maps(const float *__restrict__ mapx, const float *__restrict__ mapy, int n, int nn,
                                                      u32 *__restrict__ xy, uint16_t *__restrict__ alpha)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int x, y, a = 0;
    if (nn) {
        x = remap_sat16(remap_round(mapx[i]));
        y = remap_sat16(remap_round(mapy[i]));
    } else {
        const int sx = remap_round(mapx[i] * 32.0f), sy = remap_round(mapy[i] * 32.0f);
        x = remap_sat16(sx >> 5);
        y = remap_sat16(sy >> 5);
        a = (sy & 31) * 32 + (sx & 31);
    }
    xy[i] = (u32)(x & 0xFFFF) | (u32)(y & 0xFFFF) << 16;
    alpha[i] = (uint16_t)a;
}

// one remap launch for n frames of equal geometry on stream st.  channels / gray: 1 -> gray plane, 3 + gray -> the stage
// (gray output), 3 -> 3-channel output
static int remap_launch(hipStream_t st, const RemapFrames &F, int n, const RemapGeom &g, int channels, bool gray, int flags)
{
    bool aligned = g.dw % 4 == 0;
    for (int f = 0; f < n; ++f) aligned = aligned && ((uintptr_t)F.xy[f]) % 16 == 0 && ((uintptr_t)F.alpha[f]) % 8 == 0;
    const int quads = (g.dw + 3) / 4;
    auto kern = channels == 1 ? (aligned ? k_remap_u8<1, false, true> : k_remap_u8<1, false, false>)
                : gray        ? (aligned ? k_remap_u8<3, true, true> : k_remap_u8<3, true, false>)
                              : (aligned ? k_remap_u8<3, false, true> : k_remap_u8<3, false, false>);
    hipLaunchKernelGGL(kern, dim3((quads * g.dh + 255) / 256, n), dim3(256), 0, st, F, g, flags);
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

// depth (uint16 millimetres, dense rows of w) of a context with a rectification map through the map, nearest, border 0 =
// "no depth", into the context's depth plane (reloc_record_frame, reloc_tick_accumulate_dev)
int rectify_depth(reloc_ctx *ctx, const uint16_t *depth_dev, int w, int h, const uint16_t **out)
{
    if (w != ctx->rect_w || h != ctx->rect_h) {
        reloc_set_error("frame %dx%d differs from the rectification map %dx%d (reloc_set_rectify_map)", w, h, ctx->rect_w, ctx->rect_h);
        return RELOC_E_ARG;
    }
    RemapFrames F = {};
    F.src[0] = (const uint8_t *)depth_dev; F.xy[0] = ctx->rect_xy; F.dst[0] = (uint8_t *)ctx->rect_depth;
    const RemapGeom g = {w, h, w, w, h, w, 0};
    hipLaunchKernelGGL((k_remap_nearest<uint16_t, 1>), dim3((w + 255) / 256, 1, h), dim3(256), 0, ctx->stream, F, g);
    HIP_TRY(hipGetLastError());
    *out = ctx->rect_depth;
    return RELOC_OK;
}

// ---- resize: cv2.resize (include/reloc_spec.h, "RESIZE") ---------------------------------------------------
// OpenCV's 8-bit resize.  The per-axis tables (offsets, coefficients, tap lists) are built on the host exactly as the spec
// states them (resize_plan); the kernels do integer or f32 arithmetic on table entries only, so host and device cannot
// disagree on a floor.
//   k_resize_area<CH, GRAY, KIND>  INTER_AREA, downscale: 4 adjacent output pixels per lane.  KIND: exact 2x2 boxes, integer
//                                  iscale_x x iscale_y boxes (partial boxes at the right / bottom edge included), or per-axis
//                                  tap lists (first tap, count, f32 alphas).  GRAY (CH = 3): gray_fixed of every source pixel
//                                  before the sum, one dword store -- the stage in front of ORB.
//   k_resize_linear<CH>            INTER_LINEAR, 11 coefficient bits, one output pixel per lane
//   k_resize_nearest<T, CH>        INTER_NEAREST, one output pixel per lane; T = uint16_t for the depth image
// All are frame-batched (blockIdx.y = frame) with per-frame table pointers; a single frame is a batch of one.
enum { RESIZE_AREA_2X2 = 0, RESIZE_AREA_INT = 1, RESIZE_AREA_TAB = 2, RESIZE_LINEAR = 3, RESIZE_NEAREST = 4 };
struct ResizeFrames {
    const uint8_t *src[RELOC_BATCH_MAX]; const int32_t *tab[RELOC_BATCH_MAX]; uint8_t *dst[RELOC_BATCH_MAX];
};
struct ResizeGeom {
    int sw, sh, sstride;   // source size, row stride in bytes (k_resize_nearest: in elements of T)
    int dw, dh, dstride;   // destination size and row stride, likewise
    int isx, isy;          // integer kinds: the box
    float inv_area;        // 1.f / (isx * isy)
    int aligned;           // source rows start on dwords (base and stride multiples of 4; integer kind: isx % 4 == 0 as well)
};

// saturate_cast<uchar>(float): cvRound (half to even), then the clamp
__device__ __forceinline__ int resize_sat_u8(float v)
{
    const int r = (int)rintf(v);
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// byte b of a row segment held as dwords (b is a constant after unrolling)
#define RESIZE_BYTE(w, b) (int)(((w)[(b) >> 2] >> (8 * ((b) & 3))) & 255u)

// NW dwords of a source row from p, of which `valid` bytes belong to the row; the rest reads as 0.  aligned: p is a
// multiple of 4 and so is the row stride, so a dword that holds a valid byte ends within the row's stride
template <int NW>
__device__ __forceinline__ void resize_row_words(const uint8_t *__restrict__ p, int valid, bool aligned, u32 (&w)[NW])
{
    if (aligned) {
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = 4 * i < valid ? reinterpret_cast<const u32 *>(p)[i] : 0u;
    } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            u32 v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * i + b < valid) v |= (u32)p[4 * i + b] << (8 * b);
            w[i] = v;
        }
    }
}

// pixel j of a row segment held as dwords
template <int CH, bool GRAY, int NW>
__device__ __forceinline__ void resize_word_px(const u32 (&w)[NW], int j, int flags, int (&v)[GRAY ? 1 : CH])
{
    if (GRAY) {
        const int c0 = RESIZE_BYTE(w, 3 * j), c1 = RESIZE_BYTE(w, 3 * j + 1), c2 = RESIZE_BYTE(w, 3 * j + 2);
        v[0] = gray_fixed((flags & 1) ? c2 : c0, c1, (flags & 1) ? c0 : c2, flags);
    } else {
#pragma unroll
        for (int c = 0; c < CH; ++c) v[c] = RESIZE_BYTE(w, CH * j + c);
    }
}

// the pixel at p, byte by byte
template <int CH, bool GRAY>
__device__ __forceinline__ void resize_px(const uint8_t *__restrict__ p, int flags, int (&v)[GRAY ? 1 : CH])
{
    if (GRAY) {
        const int c0 = p[0], c1 = p[1], c2 = p[2];
        v[0] = gray_fixed((flags & 1) ? c2 : c0, c1, (flags & 1) ? c0 : c2, flags);
    } else {
#pragma unroll
        for (int c = 0; c < CH; ++c) v[c] = p[c];
    }
}

template <int CH, bool GRAY, int KIND>
__global__ __launch_bounds__(256) void k_resize_area(ResizeFrames F, ResizeGeom g, int flags)
{
    constexpr int OC = GRAY ? 1 : CH;       // output channels
    const int quads = (g.dw + 3) >> 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= quads * g.dh) return;
    const int y = q / quads, x4 = 4 * (q - y * quads);
    const uint8_t *src = F.src[blockIdx.y];
    int out[4][OC];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < OC; ++c) out[k][c] = 0;
    if (KIND == RESIZE_AREA_2X2) {
        // every box lies inside the source (2 dw <= sw, 2 dh <= sh): (a + b + c + d + 2) >> 2.  Eight source pixels per row
        constexpr int NW = 2 * CH;
        const int valid = (g.sw - 2 * x4) * CH;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            u32 w[NW];
            resize_row_words<NW>(src + (size_t)(2 * y + r) * g.sstride + (size_t)2 * x4 * CH, valid, g.aligned, w);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int v[OC];
                resize_word_px<CH, GRAY, NW>(w, j, flags, v);
#pragma unroll
                for (int c = 0; c < OC; ++c) out[j >> 1][c] += v[c];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < OC; ++c) out[k][c] = (out[k][c] + 2) >> 2;
    } else if (KIND == RESIZE_AREA_INT) {
        const int y0 = y * g.isy, ny = max(0, min(g.isy, g.sh - y0));
        const bool is22 = g.isx == 2 && g.isy == 2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x0 = (x4 + k) * g.isx, nx = x4 + k < g.dw ? max(0, min(g.isx, g.sw - x0)) : 0;
            const int count = nx * ny;
            if (count == 0) continue;           // a box that starts outside the source: 0
            int sum[OC];
#pragma unroll
            for (int c = 0; c < OC; ++c) sum[c] = 0;
            for (int r = 0; r < ny; ++r) {
                const uint8_t *row = src + (size_t)(y0 + r) * g.sstride + (size_t)x0 * CH;
                if (g.aligned && nx == g.isx) {     // isx % 4 == 0: groups of four pixels = CH dwords
                    for (int j = 0; j < nx; j += 4) {
                        u32 w[CH];
#pragma unroll
                        for (int i = 0; i < CH; ++i) w[i] = reinterpret_cast<const u32 *>(row + (size_t)j * CH)[i];
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            int v[OC];
                            resize_word_px<CH, GRAY, CH>(w, p, flags, v);
#pragma unroll
                            for (int c = 0; c < OC; ++c) sum[c] += v[c];
                        }
                    }
                } else {
                    for (int j = 0; j < nx; ++j) {
                        int v[OC];
                        resize_px<CH, GRAY>(row + (size_t)j * CH, flags, v);
#pragma unroll
                        for (int c = 0; c < OC; ++c) sum[c] += v[c];
                    }
                }
            }
            const bool inside = nx == g.isx && ny == g.isy;
#pragma unroll
            for (int c = 0; c < OC; ++c) {
                if (inside) out[k][c] = is22 ? (sum[c] + 2) >> 2 : resize_sat_u8(__fmul_rn((float)sum[c], g.inv_area));
                else        out[k][c] = resize_sat_u8(__fdiv_rn((float)sum[c], (float)count));
            }
        }
    } else {
        // tap lists: [x first dw][x count dw][x alpha offset dw][y first dh][y count dh][y alpha offset dh][f32 alphas]
        const int32_t *tab = F.tab[blockIdx.y];
        const float *al = reinterpret_cast<const float *>(tab);
        const int32_t *ty = tab + 3 * g.dw;
        const int yf = ty[y], yc = ty[g.dh + y], ya = ty[2 * g.dh + y];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (x4 + k >= g.dw) continue;
            const int xf = tab[x4 + k], xc = tab[g.dw + x4 + k], xa = tab[2 * g.dw + x4 + k];
            float acc[OC];
#pragma unroll
            for (int c = 0; c < OC; ++c) acc[c] = 0.f;
            for (int t = 0; t < yc; ++t) {
                const float beta = al[ya + t];
                const uint8_t *row = src + (size_t)(yf + t) * g.sstride + (size_t)xf * CH;
                float buf[OC];
#pragma unroll
                for (int c = 0; c < OC; ++c) buf[c] = 0.f;
                for (int u = 0; u < xc; ++u) {
                    const float a = al[xa + u];
                    int v[OC];
                    resize_px<CH, GRAY>(row + (size_t)u * CH, flags, v);
#pragma unroll
                    for (int c = 0; c < OC; ++c) buf[c] = __fadd_rn(buf[c], __fmul_rn((float)v[c], a));
                }
#pragma unroll
                for (int c = 0; c < OC; ++c) acc[c] = t == 0 ? __fmul_rn(beta, buf[c]) : __fadd_rn(acc[c], __fmul_rn(beta, buf[c]));
            }
#pragma unroll
            for (int c = 0; c < OC; ++c) out[k][c] = resize_sat_u8(acc[c]);
        }
    }
    uint8_t *dst = F.dst[blockIdx.y] + (size_t)y * g.dstride + OC * x4;
    if (OC == 1 && (g.dstride & 3) == 0) {
        // the row holds round4(dw) bytes: dstride >= dw and a multiple of 4
        *reinterpret_cast<u32 *>(dst) = (u32)out[0][0] | (u32)out[1][0] << 8 | (u32)out[2][0] << 16 | (u32)out[3][0] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x4 + k < g.dw) {
#pragma unroll
                for (int c = 0; c < OC; ++c) dst[OC * k + c] = (uint8_t)out[k][c];
            }
    }
}

// table: [x offset dw][a0 | a1 << 16 dw][row 0 dh][row 1 dh][b0 | b1 << 16 dh], the rows already clipped to the source
template <int CH>
__global__ __launch_bounds__(256) void k_resize_linear(ResizeFrames F, ResizeGeom g)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.z;
    if (x >= g.dw) return;
    const int32_t *tab = F.tab[blockIdx.y], *ty = tab + 2 * g.dw;
    const int sx = tab[x], sx1 = min(sx + 1, g.sw - 1);
    const u32 ca = (u32)tab[g.dw + x], cb = (u32)ty[2 * g.dh + y];
    const int a0 = ca & 0xFFFF, a1 = ca >> 16, b0 = cb & 0xFFFF, b1 = cb >> 16;
    const uint8_t *r0 = F.src[blockIdx.y] + (size_t)ty[y] * g.sstride, *r1 = F.src[blockIdx.y] + (size_t)ty[g.dh + y] * g.sstride;
    uint8_t *d = F.dst[blockIdx.y] + (size_t)y * g.dstride + CH * x;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int h0 = r0[CH * sx + c] * a0 + r0[CH * sx1 + c] * a1, h1 = r1[CH * sx + c] * a0 + r1[CH * sx1 + c] * a1;
        d[c] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
    }
}

// table: [x offset dw][y offset dh]; strides of src and dst in elements of T
template <typename T, int CH>
__global__ __launch_bounds__(256) void k_resize_nearest(ResizeFrames F, ResizeGeom g)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.z;
    if (x >= g.dw) return;
    const int32_t *tab = F.tab[blockIdx.y];
    const T *s = reinterpret_cast<const T *>(F.src[blockIdx.y]) + (size_t)tab[g.dw + y] * g.sstride + CH * tab[x];
    T *d = reinterpret_cast<T *>(F.dst[blockIdx.y]) + (size_t)y * g.dstride + CH * x;
#pragma unroll
    for (int c = 0; c < CH; ++c) d[c] = s[c];
}

// What one resize does: the kernel kind, the integer box and the table words (host).  Built from the spec's rules in double
// with alphas stored as f32; every source index in a table lies inside the source.
struct ResizePlan {
    int kind = -1, isx = 1, isy = 1;
    std::vector<int32_t> tab;
};

static inline int32_t resize_f32_bits(float v) { int32_t b; memcpy(&b, &v, 4); return b; }
static inline int resize_clampi(double v, int lo, int hi) { return v < (double)lo ? lo : (v > (double)hi ? hi : (int)v); }

// INTER_AREA tap list of one axis, appended to `first`, `count`, `alpha` (offsets into alpha are per axis)
static void resize_area_axis(int ss, int ds, double scale, std::vector<int32_t> &first, std::vector<int32_t> &count,
                             std::vector<int32_t> &aoff, std::vector<float> &alpha)
{
    for (int d = 0; d < ds; ++d) {
        const double f1 = d * scale, f2 = f1 + scale, cell = std::min(scale, ss - f1);
        int s1 = resize_clampi(ceil(f1), 0, ss - 1);
        const int s2 = std::min(resize_clampi(floor(f2), 0, ss), ss - 1);
        s1 = std::min(s1, s2);
        const size_t a0 = alpha.size();
        int f = s1;
        if (s1 - f1 > 1e-3 && s1 >= 1) { f = s1 - 1; alpha.push_back((float)((s1 - f1) / cell)); }
        for (int s = s1; s < s2; ++s) alpha.push_back((float)(1.0 / cell));
        if (f2 - s2 > 1e-3) alpha.push_back((float)(std::min(std::min(f2 - s2, 1.0), cell) / cell));
        first.push_back(f);
        count.push_back((int32_t)(alpha.size() - a0));
        aoff.push_back((int32_t)a0);
    }
}

// INTER_LINEAR of one axis: source index (not clipped) and the 11-bit weights of it and of its successor
static void resize_linear_axis(int ss, int ds, double scale, bool zero_at_edges, std::vector<int32_t> &ofs, std::vector<int32_t> &coef)
{
    for (int d = 0; d < ds; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        const float fl = floorf(f);
        int s = resize_clampi((double)fl, -2, ss);      // an index outside [-1, ss - 1] behaves like the nearest edge
        f -= fl;
        if (zero_at_edges) {
            if (s < 0) { s = 0; f = 0.f; }
            if (s >= ss - 1) { s = ss - 1; f = 0.f; }
        }
        const int c0 = (int)lrintf((1.f - f) * 2048.f), c1 = (int)lrintf(f * 2048.f);
        ofs.push_back(s);
        coef.push_back((int32_t)((uint32_t)(c0 & 0xFFFF) | (uint32_t)(c1 & 0xFFFF) << 16));
    }
}

static int resize_plan(int sw, int sh, int dw, int dh, double inv_x, double inv_y, int interpolation, ResizePlan &P)
{
    if (inv_x == 0.0) inv_x = (double)dw / sw;
    if (inv_y == 0.0) inv_y = (double)dh / sh;
    if (!(inv_x > 0.0 && inv_y > 0.0 && inv_x - inv_x == 0.0 && inv_y - inv_y == 0.0)) {
        reloc_set_error("bad argument: resize: the scale factors must be positive and finite");
        return RELOC_E_ARG;
    }
    const double scx = 1.0 / inv_x, scy = 1.0 / inv_y;
    std::vector<int32_t> &T = P.tab;
    T.clear();
    if (interpolation == 0) {
        P.kind = RESIZE_NEAREST;
        for (int d = 0; d < dw; ++d) T.push_back(resize_clampi(floor(d * scx), 0, sw - 1));
        for (int d = 0; d < dh; ++d) T.push_back(resize_clampi(floor(d * scy), 0, sh - 1));
        return RELOC_OK;
    }
    const int isx = resize_clampi(rint(scx), 0, 1 << 30), isy = resize_clampi(rint(scy), 0, 1 << 30);
    const bool area_fast = fabs(scx - isx) < DBL_EPSILON && fabs(scy - isy) < DBL_EPSILON;
    if (interpolation == 1 && area_fast && isx == 2 && isy == 2) interpolation = 3;
    if (interpolation == 3) {
        if (!(scx >= 1.0 && scy >= 1.0)) {
            reloc_set_error("bad argument: resize: INTER_AREA is implemented for downscaling on both axes only");
            return RELOC_E_ARG;
        }
        if (scx > 2.0 * sw || scy > 2.0 * sh) {     // no destination size rounds to >= 1 from such a factor
            reloc_set_error("bad argument: resize: INTER_AREA: a scale factor shrinks the source below half a pixel");
            return RELOC_E_ARG;
        }
        if (area_fast) {
            P.isx = isx; P.isy = isy;
            P.kind = isx == 2 && isy == 2 && 2 * (int64_t)dw <= sw && 2 * (int64_t)dh <= sh ? RESIZE_AREA_2X2 : RESIZE_AREA_INT;
            return RELOC_OK;
        }
        if ((dw - 1) * scx >= sw || (dh - 1) * scy >= sh) {
            reloc_set_error("bad argument: resize: INTER_AREA: the destination reaches beyond the scaled source");
            return RELOC_E_ARG;
        }
        P.kind = RESIZE_AREA_TAB;
        std::vector<int32_t> xf, xc, xa, yf, yc, ya;
        std::vector<float> ax, ay;
        resize_area_axis(sw, dw, scx, xf, xc, xa, ax);
        resize_area_axis(sh, dh, scy, yf, yc, ya, ay);
        const int32_t base_x = 3 * (dw + dh), base_y = base_x + (int32_t)ax.size();
        for (int d = 0; d < dw; ++d) { xa[d] += base_x; if (xf[d] + xc[d] > sw) xc[d] = sw - xf[d]; }
        for (int d = 0; d < dh; ++d) { ya[d] += base_y; if (yf[d] + yc[d] > sh) yc[d] = sh - yf[d]; }
        for (auto *v : {&xf, &xc, &xa, &yf, &yc, &ya}) T.insert(T.end(), v->begin(), v->end());
        for (float a : ax) T.push_back(resize_f32_bits(a));
        for (float a : ay) T.push_back(resize_f32_bits(a));
        return RELOC_OK;
    }
    if (interpolation == 1) {
        P.kind = RESIZE_LINEAR;
        std::vector<int32_t> xo, xc, yo, yc;
        resize_linear_axis(sw, dw, scx, true, xo, xc);
        resize_linear_axis(sh, dh, scy, false, yo, yc);
        T.insert(T.end(), xo.begin(), xo.end());
        T.insert(T.end(), xc.begin(), xc.end());
        for (int d = 0; d < dh; ++d) T.push_back(std::min(std::max(yo[d], 0), sh - 1));
        for (int d = 0; d < dh; ++d) T.push_back(std::min(std::max(yo[d] + 1, 0), sh - 1));
        T.insert(T.end(), yc.begin(), yc.end());
        return RELOC_OK;
    }
    reloc_set_error("bad argument: resize: only INTER_NEAREST (0), INTER_LINEAR (1) and INTER_AREA (3) are implemented");
    return RELOC_E_ARG;
}

// one resize launch for n frames of equal geometry on stream st.  elem: bytes per channel value (2 = the 16-bit nearest);
// gray: 3-channel source, gray output (the stage, area kinds only)
static int resize_launch(hipStream_t st, const ResizeFrames &F, int n, const ResizePlan &P, int sw, int sh, int sstride, int dw,
                         int dh, int dstride, int channels, int elem, bool gray, int flags)
{
    ResizeGeom g = {sw, sh, sstride, dw, dh, dstride, P.isx, P.isy, 1.f / (float)(P.isx * P.isy), 0};
    if (P.kind == RESIZE_NEAREST) {
        auto kern = elem == 2 ? k_resize_nearest<uint16_t, 1> : channels == 1 ? k_resize_nearest<uint8_t, 1> : k_resize_nearest<uint8_t, 3>;
        hipLaunchKernelGGL(kern, dim3((dw + 255) / 256, n, dh), dim3(256), 0, st, F, g);
    } else if (P.kind == RESIZE_LINEAR) {
        hipLaunchKernelGGL(channels == 1 ? k_resize_linear<1> : k_resize_linear<3>, dim3((dw + 255) / 256, n, dh), dim3(256), 0, st, F, g);
    } else {
        bool aligned = sstride % 4 == 0 && (P.kind != RESIZE_AREA_INT || P.isx % 4 == 0);
        for (int f = 0; f < n; ++f) aligned = aligned && ((uintptr_t)F.src[f]) % 4 == 0;
        g.aligned = aligned;
        const dim3 grid((((dw + 3) / 4) * dh + 255) / 256, n);
#define RESIZE_AREA_KERN(KIND) (channels == 1 ? k_resize_area<1, false, KIND> : gray ? k_resize_area<3, true, KIND> : k_resize_area<3, false, KIND>)
        auto kern = P.kind == RESIZE_AREA_2X2 ? RESIZE_AREA_KERN(RESIZE_AREA_2X2)
                    : P.kind == RESIZE_AREA_INT ? RESIZE_AREA_KERN(RESIZE_AREA_INT) : RESIZE_AREA_KERN(RESIZE_AREA_TAB);
#undef RESIZE_AREA_KERN
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, F, g, flags);
    }
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

// depth (uint16 millimetres, dense rows of w) of a context with the downscale stage on, INTER_NEAREST to the working size,
// into the context's depth plane (reloc_record_frame, reloc_tick_accumulate_dev)
int resize_depth(reloc_ctx *ctx, const uint16_t *depth_dev, int w, int h, const uint16_t **out)
{
    if (w != ctx->rsz_sw || h != ctx->rsz_sh) {
        reloc_set_error("frame %dx%d differs from the source size %dx%d of the downscale stage (reloc_set_resize)", w, h, ctx->rsz_sw, ctx->rsz_sh);
        return RELOC_E_ARG;
    }
    ResizeFrames F = {};
    F.src[0] = (const uint8_t *)depth_dev; F.tab[0] = ctx->rsz_ntab; F.dst[0] = (uint8_t *)ctx->rsz_depth;
    ResizePlan P;
    P.kind = RESIZE_NEAREST;
    if (int rc = resize_launch(ctx->stream, F, 1, P, w, h, w, ctx->rsz_dw, ctx->rsz_dh, ctx->rsz_dw, 1, 2, false, 0)) return rc;
    *out = ctx->rsz_depth;
    return RELOC_OK;
}

// what the five ORB kernels read and write of a context, for the source frame src
static OrbFrame orb_frame(const reloc_ctx *c, const uint8_t *src)
{
    OrbFrame F;
    F.tab = (const OrbTable *)c->orb_const; F.tiles = (const PyrTile *)c->pyr_tiles; F.rz = c->rz_tab; F.src = src;
    F.pyr = c->pyr; F.nms = c->nms; F.blur = c->blur; F.hist = c->hist; F.cand_cnt = c->cand_cnt; F.cand_key = c->cand_key;
    F.cand_resp = c->cand_resp; F.dbg_cut = c->dbg_cut; F.kp_cnt = c->kp_cnt; F.kp_key = c->kp_key; F.kp_resp = c->kp_resp;
    F.f_xy = c->f_xy; F.f_size = c->f_size; F.f_angle = c->f_angle; F.f_resp = c->f_resp; F.f_oct = c->f_oct; F.f_desc = c->f_desc;
    F.f_count = c->f_count;
    return F;
}

// Five launches (plus one of the downscale stage, one of the rectification and two of CLAHE): the frames are of equal
// geometry.  3-channel frames of contexts with the downscale stage on (reloc_set_resize) are converted to gray and resized
// (INTER_AREA) first, and everything downstream sees the working frame dw x dh; those of
// contexts with a rectification map (reloc_set_rectify_map) are converted to gray and remapped first, those of contexts
// with CLAHE on (reloc_set_clahe) equalised next; the pyramid then reads the last plane written.  The pyramid runs 512-thread workgroups
// for latency, 256 where it shares the chip with whole-database scans.
int orb_run(reloc_ctx *const *ctxs, int n, const uint8_t *const *srcs, int w, int h, int stride, int channels, int order,
            int nfeatures, bool latency)
{
    if (n < 1 || n > RELOC_BATCH_MAX) { reloc_set_error("orb: 1..%d frames", RELOC_BATCH_MAX); return RELOC_E_ARG; }
    reloc_ctx *c0 = ctxs[0];
    const bool frame = channels == 3;      // the image stages serve 3-channel frames only, never a caller's gray plane
    const bool resize = frame && c0->rsz_dw > 0;
    const int sw = w, sh = h;               // the frame as handed in; w x h becomes the working frame
    for (int f = 0; f < n; ++f) {
        const reloc_ctx *c = ctxs[f];
        if (c->rsz_sw != c0->rsz_sw || c->rsz_sh != c0->rsz_sh || c->rsz_dw != c0->rsz_dw || c->rsz_dh != c0->rsz_dh) {
            reloc_set_error("orb batch: contexts with and without the downscale stage, or with unequal sizes (reloc_set_resize)");
            return RELOC_E_STATE;
        }
    }
    if (resize) {
        if (w != c0->rsz_sw || h != c0->rsz_sh) {
            reloc_set_error("frame %dx%d differs from the source size %dx%d of the downscale stage (reloc_set_resize)", w, h, c0->rsz_sw, c0->rsz_sh);
            return RELOC_E_ARG;
        }
        w = c0->rsz_dw; h = c0->rsz_dh;
        if (w < 64 || h < 64) { reloc_set_error("bad argument: the working frame %dx%d of the downscale stage is below 64x64", w, h); return RELOC_E_ARG; }
    }
    for (int f = 0; f < n; ++f) {
        reloc_ctx *c = ctxs[f];
        if (int rc = orb_prepare(c, w, h, nfeatures)) return rc;
        if (c->pyr_ntiles != c0->pyr_ntiles || c->pyr_lds_bytes != c0->pyr_lds_bytes || c->max_feat != c0->max_feat ||
            c->prm.gray_coeff_bits != c0->prm.gray_coeff_bits) {
            reloc_set_error("orb batch: contexts of unequal geometry");
            return RELOC_E_STATE;
        }
        if (c->rect_w != c0->rect_w || c->rect_h != c0->rect_h) {
            reloc_set_error("orb batch: contexts with and without a rectification map, or with maps of unequal size (reloc_set_rectify_map)");
            return RELOC_E_STATE;
        }
        if (c->clahe_tx != c0->clahe_tx || c->clahe_ty != c0->clahe_ty || c->clahe_clip != c0->clahe_clip) {
            reloc_set_error("orb batch: contexts of unequal CLAHE settings (reloc_set_clahe)");
            return RELOC_E_STATE;
        }
    }
    if (frame && c0->rect_w > 0 && (w != c0->rect_w || h != c0->rect_h)) {
        reloc_set_error("frame %dx%d differs from the rectification map %dx%d (reloc_set_rectify_map)", w, h, c0->rect_w, c0->rect_h);
        return RELOC_E_ARG;
    }
    const OrbTable *tab_h = (const OrbTable *)c0->orb_tab_host;
    const int flags = gray_flags(c0, order);
    hipStream_t st = c0->stream;
    reloc_prof_begin(c0, RELOC_PROF_ORB);
    const uint8_t *zplanes[RELOC_BATCH_MAX], *rplanes[RELOC_BATCH_MAX], *planes[RELOC_BATCH_MAX];
    if (resize) {
        ResizeFrames F = {};
        for (int f = 0; f < n; ++f) { F.src[f] = srcs[f]; F.tab[f] = ctxs[f]->rsz_tab; F.dst[f] = ctxs[f]->rsz_plane; zplanes[f] = F.dst[f]; }
        ResizePlan P;
        P.kind = c0->rsz_kind; P.isx = c0->rsz_isx; P.isy = c0->rsz_isy;
        const int cs = clahe_stride(w);
        if (int rc = resize_launch(st, F, n, P, sw, sh, stride, w, h, cs, 3, 1, true, flags)) {
            reloc_prof_end(c0, RELOC_PROF_ORB);
            return rc;
        }
        srcs = zplanes; stride = cs; channels = 1;
    }
    if (frame && c0->rect_w > 0) {
        RemapFrames F = {};
        for (int f = 0; f < n; ++f) {
            F.src[f] = srcs[f]; F.xy[f] = ctxs[f]->rect_xy; F.alpha[f] = ctxs[f]->rect_alpha; F.dst[f] = ctxs[f]->rect_plane;
            rplanes[f] = F.dst[f];
        }
        const int cs = clahe_stride(w);
        const RemapGeom g = {w, h, stride, w, h, cs, 0};
        if (int rc = remap_launch(st, F, n, g, channels, channels == 3, flags)) {
            reloc_prof_end(c0, RELOC_PROF_ORB);
            return rc;
        }
        srcs = rplanes; stride = cs; channels = 1;
    }
    if (frame && c0->clahe_tx > 0) {
        ClaheFrames F = {};
        for (int f = 0; f < n; ++f) { F.src[f] = srcs[f]; F.lut[f] = ctxs[f]->clahe_lut; F.dst[f] = ctxs[f]->clahe_plane; planes[f] = F.dst[f]; }
        const int cs = clahe_stride(w);
        if (int rc = clahe_launch(st, F, n, clahe_geom(w, h, c0->clahe_clip, c0->clahe_tx, c0->clahe_ty), channels, stride, flags, cs)) {
            reloc_prof_end(c0, RELOC_PROF_ORB);
            return rc;
        }
        srcs = planes; stride = cs; channels = 1;
    }
    bool aligned = w % 4 == 0 && stride % 4 == 0;
    for (int f = 0; f < n; ++f) aligned = aligned && ((uintptr_t)srcs[f]) % 4 == 0;
    OrbBatch b;
    frame_slots(ctxs, n, [&](int f, reloc_ctx *c, int g) { b.f[f] = orb_frame(c, srcs[g]); });
    PyrLds lds;
    for (int l = 0; l < NLEV; ++l) lds.lev[l] = c0->pyr_lds[l];
    lds.tabs = c0->pyr_lds[NLEV];
    const int n_fast = tab_h->fast_tile_base[NLEV], n_blur = tab_h->blur_tile_base[NLEV];
    if (n == 1) {
        const OrbFrame &F = b.f[0];
        auto kern512 = channels == 3 ? (aligned ? k_pyramid<3, true, 512> : k_pyramid<3, false, 512>) : (aligned ? k_pyramid<1, true, 512> : k_pyramid<1, false, 512>);
        auto kern256 = channels == 3 ? (aligned ? k_pyramid<3, true, 256> : k_pyramid<3, false, 256>) : (aligned ? k_pyramid<1, true, 256> : k_pyramid<1, false, 256>);
        hipLaunchKernelGGL(latency ? kern512 : kern256, dim3(c0->pyr_ntiles), dim3(latency ? 512 : 256), c0->pyr_lds_bytes, st, F.tab,
                           F.tiles, F.rz, F.src, w, h, stride, flags, F.pyr, lds, F.hist, F.cand_cnt);
        hipLaunchKernelGGL(k_fast_blur, dim3(n_fast + n_blur), dim3(256), 0, st, F.tab, F.pyr, F.nms, F.hist, F.blur, n_fast);
        hipLaunchKernelGGL(k_harris, dim3(tab_h->flat_base[NLEV]), dim3(256), 0, st, F.tab, F.pyr, F.nms, F.hist, F.cand_cnt, F.cand_key,
                           F.cand_resp, F.dbg_cut);
        hipLaunchKernelGGL(k_select, dim3(NLEV), dim3(1024), 0, st, F.tab, F.cand_cnt, F.cand_key, F.cand_resp, F.kp_cnt, F.kp_key,
                           F.kp_resp);
        hipLaunchKernelGGL(k_describe, dim3((c0->max_feat + 3) / 4), dim3(256), 0, st, F.tab, F.pyr, F.blur, F.kp_cnt, F.kp_key,
                           F.kp_resp, c0->max_feat, F.f_xy, F.f_size, F.f_angle, F.f_resp, F.f_oct, F.f_desc, F.f_count);
    } else {
        auto kern = channels == 3 ? (aligned ? k_pyramid_batch<3, true, 256> : k_pyramid_batch<3, false, 256>)
                                  : (aligned ? k_pyramid_batch<1, true, 256> : k_pyramid_batch<1, false, 256>);
        hipLaunchKernelGGL(kern, dim3(c0->pyr_ntiles, n), dim3(256), c0->pyr_lds_bytes, st, b, w, h, stride, flags, lds);
        hipLaunchKernelGGL(k_fast_blur_batch, dim3(n_fast + n_blur, n), dim3(256), 0, st, b, n_fast);
        hipLaunchKernelGGL(k_harris_batch, dim3(tab_h->flat_base[NLEV], n), dim3(256), 0, st, b);
        hipLaunchKernelGGL(k_select_batch, dim3(NLEV, n), dim3(1024), 0, st, b);
        hipLaunchKernelGGL(k_describe_batch, dim3((c0->max_feat + 3) / 4, n), dim3(256), 0, st, b, c0->max_feat);
    }
    reloc_prof_end(c0, RELOC_PROF_ORB);
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}


// ------------------------------------------------------------------------------------------------
RELOC_API int reloc_gray_u8(reloc_ctx *ctx, const uint8_t *img, int w, int h, int stride, int order, uint8_t *gray)
{
    ARG_CHECK_CTX(ctx, img && gray && w > 0 && h > 0 && stride >= 3 * w, "reloc_gray_u8");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    void *dout;
    int rc;
    if ((rc = reloc_scratch(ctx, 0, (int64_t)w * h, &dout))) return rc;
    HIP_TRY(hipMemcpy2DAsync(ctx->frame_img, (size_t)w * 3, img, stride, (size_t)w * 3, h, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_gray_plain, dim3((w + 255) / 256, h), dim3(256), 0, ctx->stream, ctx->frame_img, w, h, w * 3, gray_flags(ctx, order),
                       (uint8_t *)dout);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(gray, dout, (size_t)w * h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RELOC_OK;
}

RELOC_API int reloc_orb_frame_dev(reloc_ctx *ctx, const uint8_t *img_dev, int w, int h, int stride, int order, int nfeatures)
{
    ARG_CHECK_CTX(ctx, img_dev && w >= 64 && h >= 64 && stride >= 3 * w && nfeatures > 0, "reloc_orb_frame_dev");
    return orb_run(&ctx, 1, &img_dev, w, h, stride, 3, order, nfeatures, true);
}

RELOC_API const uint8_t *reloc_frame_desc_dev(reloc_ctx *ctx) { return ctx ? ctx->f_desc : nullptr; }
RELOC_API const float *reloc_frame_xy_dev(reloc_ctx *ctx) { return ctx ? ctx->f_xy : nullptr; }
RELOC_API const int32_t *reloc_frame_count_dev(reloc_ctx *ctx) { return ctx ? ctx->f_count : nullptr; }

RELOC_API int reloc_orb_detect_compute(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride, int nfeatures,
                                       float *xy, float *size, float *angle, float *response, int32_t *octave,
                                       uint8_t *desc, int32_t *n_out)
{
    ARG_CHECK_CTX(ctx, gray && n_out && w > 0 && h > 0 && stride >= w && nfeatures > 0, "reloc_orb_detect_compute");
    *n_out = 0;
    if (w < 63 || h < 63) return RELOC_OK;   // no level is wider than the 31-pixel edge margin on both sides
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    HIP_TRY(hipMemcpy2DAsync(ctx->frame_img, w, gray, stride, w, h, hipMemcpyHostToDevice, ctx->stream));
    const uint8_t *src = ctx->frame_img;
    int rc = orb_run(&ctx, 1, &src, w, h, w, 1, 0, nfeatures, true);
    if (rc) return rc;
    int32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, ctx->f_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (n > 0) {
        if (xy) HIP_TRY(hipMemcpyAsync(xy, ctx->f_xy, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (size) HIP_TRY(hipMemcpyAsync(size, ctx->f_size, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (angle) HIP_TRY(hipMemcpyAsync(angle, ctx->f_angle, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (response) HIP_TRY(hipMemcpyAsync(response, ctx->f_resp, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (octave) HIP_TRY(hipMemcpyAsync(octave, ctx->f_oct, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (desc) HIP_TRY(hipMemcpyAsync(desc, ctx->f_desc, (size_t)n * 32, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    *n_out = n;
    return RELOC_OK;
}

RELOC_API int reloc_frame_debug_plane(reloc_ctx *ctx, int what, int level, uint8_t *out, int32_t *w, int32_t *h)
{
    ARG_CHECK_CTX(ctx, out && w && h && what >= 0 && what <= 2 && level >= 0 && level < NLEV, "reloc_frame_debug_plane");
    if (!ctx->orb_w) { reloc_set_error("no frame processed yet"); return RELOC_E_STATE; }
    const OrbLevel &L = ctx->lev[level];
    const uint8_t *src = (what == 0 ? ctx->pyr : what == 1 ? ctx->blur : ctx->nms) + L.off;
    HIP_TRY(hipMemcpy2DAsync(out, L.w, src, L.stride, L.w, L.h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *w = L.w;
    *h = L.h;
    return RELOC_OK;
}

// ---- CLAHE entry points -------------------------------------------------------------------------------
static bool clahe_args_ok(double clip_limit, int tiles_x, int tiles_y)
{
    return clip_limit - clip_limit == 0.0 && tiles_x >= 1 && tiles_x <= CLAHE_MAX_TILES && tiles_y >= 1 && tiles_y <= CLAHE_MAX_TILES;
}

RELOC_API int reloc_set_clahe(reloc_ctx *ctx, double clip_limit, int tiles_x, int tiles_y)
{
    ARG_CHECK_CTX(ctx, true, "ctx is NULL");
    if (tiles_x == 0 && tiles_y == 0) {
        ctx->clahe_clip = 0.0;
        ctx->clahe_tx = ctx->clahe_ty = 0;
        return RELOC_OK;
    }
    ARG_CHECK(clahe_args_ok(clip_limit, tiles_x, tiles_y),
              "reloc_set_clahe: tiles_x and tiles_y must both be 0 (off) or both in 1..64, and clip_limit finite");
    if (!ctx->clahe_plane) {
        // first enable: the plane of the largest frame and the LUTs of the largest grid
        HIP_TRY(hipMalloc((void **)&ctx->clahe_plane, (size_t)clahe_stride(ctx->max_w) * ctx->max_h));
        const hipError_t e = hipMalloc((void **)&ctx->clahe_lut, (size_t)CLAHE_MAX_TILES * CLAHE_MAX_TILES * 256);
        if (e != hipSuccess) {
            (void)hipFree(ctx->clahe_plane);
            ctx->clahe_plane = nullptr;
            HIP_TRY(e);
        }
    }
    ctx->clahe_clip = clip_limit == 0.0 ? 0.0 : clip_limit;     // -0 -> +0: equal settings compare equal
    ctx->clahe_tx = tiles_x;
    ctx->clahe_ty = tiles_y;
    return RELOC_OK;
}

RELOC_API int reloc_get_clahe(reloc_ctx *ctx, double *clip_limit, int32_t *tiles_x, int32_t *tiles_y)
{
    ARG_CHECK_CTX(ctx, clip_limit && tiles_x && tiles_y, "reloc_get_clahe");
    *clip_limit = ctx->clahe_clip;
    *tiles_x = ctx->clahe_tx;
    *tiles_y = ctx->clahe_ty;
    return RELOC_OK;
}

RELOC_API int reloc_clahe_u8(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride, double clip_limit, int tiles_x,
                             int tiles_y, uint8_t *out)
{
    ARG_CHECK_CTX(ctx, gray && out && w >= 1 && h >= 1 && stride >= w, "reloc_clahe_u8");
    ARG_CHECK(clahe_args_ok(clip_limit, tiles_x, tiles_y), "reloc_clahe_u8: tiles_x, tiles_y must be in 1..64 and clip_limit finite");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    void *dlut, *dout;
    int rc;
    if ((rc = reloc_scratch(ctx, 0, (int64_t)tiles_x * tiles_y * 256, &dlut))) return rc;
    if ((rc = reloc_scratch(ctx, 1, (int64_t)w * h, &dout))) return rc;
    HIP_TRY(hipMemcpy2DAsync(ctx->frame_img, w, gray, stride, w, h, hipMemcpyHostToDevice, ctx->stream));
    ClaheFrames F = {};
    F.src[0] = ctx->frame_img; F.lut[0] = (uint8_t *)dlut; F.dst[0] = (uint8_t *)dout;
    if ((rc = clahe_launch(ctx->stream, F, 1, clahe_geom(w, h, clip_limit, tiles_x, tiles_y), 1, w, 0, w))) return rc;
    HIP_TRY(hipMemcpyAsync(out, dout, (size_t)w * h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RELOC_OK;
}

// ---- rectification entry points ----------------------------------------------------------------------------
RELOC_API int reloc_set_rectify_map(reloc_ctx *ctx, const int16_t *xy, const uint16_t *alpha, int w, int h)
{
    ARG_CHECK_CTX(ctx, true, "ctx is NULL");
    if (!xy) {
        ctx->rect_w = ctx->rect_h = 0;
        return RELOC_OK;
    }
    ARG_CHECK(alpha && w >= 1 && h >= 1, "reloc_set_rectify_map: alpha is NULL or the size is not positive");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("rectification map exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    if (!ctx->rect_xy) {
        // first enable: maps and planes of the largest frame, in one allocation (rect_xy owns it)
        const size_t px = (size_t)ctx->max_w * ctx->max_h, plane = (size_t)clahe_stride(ctx->max_w) * ctx->max_h;
        uint8_t *base;
        HIP_TRY(hipMalloc((void **)&base, px * 4 + px * 2 + px * 2 + plane));
        ctx->rect_xy = (int16_t *)base;
        ctx->rect_alpha = (uint16_t *)(base + px * 4);
        ctx->rect_depth = (uint16_t *)(base + px * 6);
        ctx->rect_plane = base + px * 8;
    }
    // frames in flight may still read the previous map
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(ctx->rect_xy, xy, (size_t)w * h * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->rect_alpha, alpha, (size_t)w * h * 2, hipMemcpyHostToDevice));
    ctx->rect_w = w;
    ctx->rect_h = h;
    return RELOC_OK;
}

RELOC_API int reloc_get_rectify_map(reloc_ctx *ctx, int32_t *w, int32_t *h)
{
    ARG_CHECK_CTX(ctx, w && h, "reloc_get_rectify_map");
    *w = ctx->rect_w;
    *h = ctx->rect_h;
    return RELOC_OK;
}

// source, maps and destination of a host-pointer remap on the device: src into frame_img (dense rows), maps into scratch 0 / 1
static int remap_stage(reloc_ctx *ctx, const void *src, int sw, int sh, int sstride, int row_bytes, const int16_t *xy,
                       const uint16_t *alpha, int dw, int dh, int64_t out_bytes, RemapFrames &F)
{
    if (sw > ctx->max_w || sh > ctx->max_h || dw > ctx->max_w || dh > ctx->max_h) {
        reloc_set_error("image or map exceeds ctx capacity");
        return RELOC_E_CAPACITY;
    }
    void *dxy, *dal, *dout;
    int rc;
    if ((rc = reloc_scratch(ctx, 0, (int64_t)dw * dh * 4, &dxy))) return rc;
    if ((rc = reloc_scratch(ctx, 1, (int64_t)dw * dh * 2, &dal))) return rc;
    if ((rc = reloc_scratch(ctx, 2, out_bytes, &dout))) return rc;
    HIP_TRY(hipMemcpy2DAsync(ctx->frame_img, row_bytes, src, sstride, row_bytes, sh, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dxy, xy, (size_t)dw * dh * 4, hipMemcpyHostToDevice, ctx->stream));
    if (alpha) HIP_TRY(hipMemcpyAsync(dal, alpha, (size_t)dw * dh * 2, hipMemcpyHostToDevice, ctx->stream));
    F = {};
    F.src[0] = ctx->frame_img; F.xy[0] = (const int16_t *)dxy; F.alpha[0] = (const uint16_t *)dal; F.dst[0] = (uint8_t *)dout;
    return RELOC_OK;
}

RELOC_API int reloc_remap_u8(reloc_ctx *ctx, const uint8_t *src, int sw, int sh, int sstride, int channels, const int16_t *xy,
                             const uint16_t *alpha, int dw, int dh, int nearest, int border_value, uint8_t *out)
{
    ARG_CHECK_CTX(ctx, src && xy && out && (alpha || nearest) && sw >= 1 && sh >= 1 && dw >= 1 && dh >= 1 &&
                  (channels == 1 || channels == 3) && sstride >= channels * sw && border_value >= 0 && border_value <= 255,
                  "reloc_remap_u8");
    RemapFrames F;
    const int64_t out_bytes = (int64_t)dw * dh * channels;
    if (int rc = remap_stage(ctx, src, sw, sh, sstride, sw * channels, xy, alpha, dw, dh, out_bytes, F)) return rc;
    const RemapGeom g = {sw, sh, sw * channels, dw, dh, dw * channels, border_value};
    if (nearest) {
        auto kern = channels == 1 ? k_remap_nearest<uint8_t, 1> : k_remap_nearest<uint8_t, 3>;
        hipLaunchKernelGGL(kern, dim3((dw + 255) / 256, 1, dh), dim3(256), 0, ctx->stream, F, g);
        HIP_TRY(hipGetLastError());
    } else if (int rc = remap_launch(ctx->stream, F, 1, g, channels, false, 0)) {
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(out, F.dst[0], (size_t)out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RELOC_OK;
}

RELOC_API int reloc_remap_u16(reloc_ctx *ctx, const uint16_t *src, int sw, int sh, int sstride, const int16_t *xy, int dw, int dh,
                              int border_value, uint16_t *out)
{
    ARG_CHECK_CTX(ctx, src && xy && out && sw >= 1 && sh >= 1 && dw >= 1 && dh >= 1 && sstride >= 2 * sw && border_value >= 0 &&
                  border_value <= 65535, "reloc_remap_u16");
    RemapFrames F;
    const int64_t out_bytes = (int64_t)dw * dh * 2;
    if (int rc = remap_stage(ctx, src, sw, sh, sstride, sw * 2, xy, nullptr, dw, dh, out_bytes, F)) return rc;
    const RemapGeom g = {sw, sh, sw, dw, dh, dw, border_value};        // strides in elements
    hipLaunchKernelGGL((k_remap_nearest<uint16_t, 1>), dim3((dw + 255) / 256, 1, dh), dim3(256), 0, ctx->stream, F, g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, F.dst[0], (size_t)out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RELOC_OK;
}

RELOC_API int reloc_convert_maps(reloc_ctx *ctx, const float *mapx, const float *mapy, int w, int h, int nninterpolation,
                                 int16_t *xy_out, uint16_t *alpha_out)
{
    ARG_CHECK_CTX(ctx, mapx && mapy && xy_out && alpha_out && w >= 1 && h >= 1, "reloc_convert_maps");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("map exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    const int64_t n = (int64_t)w * h;
    void *dmx, *dmy, *dxy, *dal;
    int rc;
    if ((rc = reloc_scratch(ctx, 0, n * 4, &dxy))) return rc;
    if ((rc = reloc_scratch(ctx, 1, n * 2, &dal))) return rc;
    if ((rc = reloc_scratch(ctx, 2, n * 4, &dmx))) return rc;
    if ((rc = reloc_scratch(ctx, 3, n * 4, &dmy))) return rc;
    HIP_TRY(hipMemcpyAsync(dmx, mapx, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dmy, mapy, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_convert_maps, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const float *)dmx,
                       (const float *)dmy, (int)n, nninterpolation, (u32 *)dxy, (uint16_t *)dal);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(xy_out, dxy, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(alpha_out, dal, (size_t)n * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RELOC_OK;
}

// ---- resize entry points -------------------------------------------------------------------------------------
// source, table and destination of a host-pointer resize on the device: src into frame_img (dense rows), table into scratch 0
static int resize_host(reloc_ctx *ctx, const void *src, int sw, int sh, int sstride, int channels, int elem, void *out, int dw, int dh,
                       double inv_x, double inv_y, int interpolation)
{
    if (sw > ctx->max_w || sh > ctx->max_h || dw > ctx->max_w || dh > ctx->max_h) {
        reloc_set_error("image exceeds ctx capacity");
        return RELOC_E_CAPACITY;
    }
    ResizePlan P;
    if (int rc = resize_plan(sw, sh, dw, dh, inv_x, inv_y, interpolation, P)) return rc;
    const int row_bytes = sw * channels * elem;
    const int64_t out_bytes = (int64_t)dw * dh * channels * elem;
    void *dtab, *dout;
    int rc;
    if ((rc = reloc_scratch(ctx, 0, (int64_t)P.tab.size() * 4 + 4, &dtab))) return rc;
    if ((rc = reloc_scratch(ctx, 1, out_bytes, &dout))) return rc;
    HIP_TRY(hipMemcpy2DAsync(ctx->frame_img, row_bytes, src, sstride, row_bytes, sh, hipMemcpyHostToDevice, ctx->stream));
    // the table is pageable host memory that dies with this call: the copy below is complete when the call returns
    if (!P.tab.empty()) HIP_TRY(hipMemcpyAsync(dtab, P.tab.data(), P.tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ResizeFrames F = {};
    F.src[0] = ctx->frame_img; F.tab[0] = (const int32_t *)dtab; F.dst[0] = (uint8_t *)dout;
    const bool by_elem = P.kind == RESIZE_NEAREST;      // k_resize_nearest counts strides in elements
    if ((rc = resize_launch(ctx->stream, F, 1, P, sw, sh, by_elem ? sw * channels : row_bytes, dw, dh, dw * channels, channels, elem,
                            false, 0)))
        return rc;
    HIP_TRY(hipMemcpyAsync(out, dout, (size_t)out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RELOC_OK;
}

RELOC_API int reloc_resize_u8(reloc_ctx *ctx, const uint8_t *src, int sw, int sh, int sstride, int channels, uint8_t *out, int dw,
                              int dh, double inv_scale_x, double inv_scale_y, int interpolation)
{
    ARG_CHECK_CTX(ctx, src && out && sw >= 1 && sh >= 1 && dw >= 1 && dh >= 1 && (channels == 1 || channels == 3) &&
                  sstride >= channels * sw, "reloc_resize_u8");
    return resize_host(ctx, src, sw, sh, sstride, channels, 1, out, dw, dh, inv_scale_x, inv_scale_y, interpolation);
}

RELOC_API int reloc_resize_u16(reloc_ctx *ctx, const uint16_t *src, int sw, int sh, int sstride, uint16_t *out, int dw, int dh,
                               double inv_scale_x, double inv_scale_y)
{
    ARG_CHECK_CTX(ctx, src && out && sw >= 1 && sh >= 1 && dw >= 1 && dh >= 1 && sstride >= 2 * sw, "reloc_resize_u16");
    return resize_host(ctx, src, sw, sh, sstride, 1, 2, out, dw, dh, inv_scale_x, inv_scale_y, 0);
}

RELOC_API int reloc_set_resize(reloc_ctx *ctx, int sw, int sh, int dw, int dh)
{
    ARG_CHECK_CTX(ctx, true, "ctx is NULL");
    if (sw == 0 && sh == 0 && dw == 0 && dh == 0) {
        ctx->rsz_sw = ctx->rsz_sh = ctx->rsz_dw = ctx->rsz_dh = 0;
        return RELOC_OK;
    }
    ARG_CHECK(dw >= 1 && dh >= 1 && dw <= sw && dh <= sh,
              "reloc_set_resize: sizes must be all 0 (off) or 1 <= dw <= sw and 1 <= dh <= sh");
    if (sw > ctx->max_w || sh > ctx->max_h) { reloc_set_error("resize source exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    ResizePlan area, nearest;
    if (int rc = resize_plan(sw, sh, dw, dh, 0.0, 0.0, 3, area)) return rc;
    if (int rc = resize_plan(sw, sh, dw, dh, 0.0, 0.0, 0, nearest)) return rc;
    // tables of the largest frame: 3 words and at most scale + 2 alphas per destination index and axis, one offset per index
    // and axis for the depth; then the gray plane and the depth plane, in one allocation (rsz_tab owns it)
    const size_t area_words = 6 * ((size_t)ctx->max_w + ctx->max_h), near_words = (size_t)ctx->max_w + ctx->max_h;
    if (area.tab.size() > area_words || nearest.tab.size() > near_words) { reloc_set_error("resize tables exceed ctx capacity"); return RELOC_E_CAPACITY; }
    if (!ctx->rsz_tab) {
        const size_t px = (size_t)ctx->max_w * ctx->max_h, plane = (size_t)clahe_stride(ctx->max_w) * ctx->max_h;
        const size_t tab_bytes = ((area_words + near_words) * 4 + 255) & ~(size_t)255;
        uint8_t *base;
        HIP_TRY(hipMalloc((void **)&base, tab_bytes + plane + px * 2));
        ctx->rsz_tab = (int32_t *)base;
        ctx->rsz_ntab = ctx->rsz_tab + area_words;
        ctx->rsz_plane = base + tab_bytes;
        ctx->rsz_depth = (uint16_t *)(base + tab_bytes + plane);
    }
    // frames in flight may still read the previous tables
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!area.tab.empty()) HIP_TRY(hipMemcpy(ctx->rsz_tab, area.tab.data(), area.tab.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->rsz_ntab, nearest.tab.data(), nearest.tab.size() * 4, hipMemcpyHostToDevice));
    ctx->rsz_kind = area.kind; ctx->rsz_isx = area.isx; ctx->rsz_isy = area.isy;
    ctx->rsz_sw = sw; ctx->rsz_sh = sh; ctx->rsz_dw = dw; ctx->rsz_dh = dh;
    return RELOC_OK;
}

RELOC_API int reloc_get_resize(reloc_ctx *ctx, int32_t *sw, int32_t *sh, int32_t *dw, int32_t *dh)
{
    ARG_CHECK_CTX(ctx, sw && sh && dw && dh, "reloc_get_resize");
    *sw = ctx->rsz_sw; *sh = ctx->rsz_sh; *dw = ctx->rsz_dw; *dh = ctx->rsz_dh;
    return RELOC_OK;
}
