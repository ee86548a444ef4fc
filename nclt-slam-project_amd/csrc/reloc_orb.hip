// reloc_orb.hip -- ORB front end on gfx950: 8-level pyramid (gray conversion fused) -> FAST-9/16 + NMS ->
// best-2n by FAST score -> Harris -> best-n -> intensity-centroid angle -> 7x7 blur -> steered
// BRIEF-256.  Serves cv2.ORB_create(nfeatures).detectAndCompute(gray, None)        (reference M:306, R:241).
// nlevels, scaleFactor, fastThreshold and scoreType are runtime parameters (include/reloc_spec.h "ORB PARAMS";
// reloc_set_orb_params, reloc_orb_detect_compute_params): the plan of a frame carries them (OrbParams, reloc_orb_plan.h), levels
// behind nlevels are empty, and the default set runs the kernels built for its constants (k_fast_blur<*, 20>, k_harris<0>).
// Holds the five ORB kernels with their batched twins, orb_alloc (the blocks of a context's OrbState, ctx->orb), orb_prepare
// (uploads the plan of a frame size: reloc_orb_plan.h holds the level, table and tile types and the host arithmetic), orb_run
// and the ORB entry points.  What happens to a frame before the pyramid is reloc_image.hip; the pixel helpers of both are
// reloc_pixels.h.
//
// Everything is integer or strictly-ordered IEEE float arithmetic (no fused multiply-add, own
// sin/cos) so results are bit-identical to the specification; the algorithm constants live in
// include/reloc_spec.h.  Data layout in HBM: every pyramid level is a plane with a 64-byte-aligned
// row stride inside one arena (ctx->orb.buf.pyr); the blurred pyramid (buf.blur) and the NMS score maps
// (buf.nms) use the same geometry, so a level is addressed by one offset in all three.
//
// The image chain feeds it through orb_run: image_chain_check, orb_prepare for the working frame, then image_chain_gray runs
// the stages that are on and names the last plane written, which k_pyramid reads instead of the caller's frame.
//
// Five launches per frame (all on the ctx stream):
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
// A detection mask (include/reloc_spec.h "ORB MASK"; reloc_set_orb_mask, reloc_orb_detect_compute_masked) adds no launch per
// frame: k_fast_blur<true> reads the frame's mask pyramid (geometry of buf.pyr) where it writes the NMS map; k_mask_level
// builds that pyramid once per mask, seven dependent launches in front of the first frame that uses it.
// The per-frame HBM traffic is about 4 MB at 640x480; the stage is launch/latency-bound, not
// bandwidth-bound.
#include <math.h>

#include "../../include/reloc_orb_pattern.h"
#include "reloc_internal.h"
#include "reloc_pixels.h"

static_assert(HARRIS_CHUNK == 1024, "k_harris reads one dword per thread");

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

// ---- fused pyramid ------------------------------------------------------------------------------
// One launch builds level 0 (gray conversion or a copy of a gray plane) AND levels 1..7.  Level l is a
// resize of level l-1; as seven launches (round 1) that was a dependent chain of tiny kernels, 4.3 us
// each, 30 us of a 75 us front end.  Here a workgroup owns one rectangle of EVERY level (`o`, 4-pixel
// aligned in x so it is stored as dwords) and computes, in LDS, the slightly larger rectangle `n` of
// each level that its rectangles of the levels above need as bilinear taps -- at most one extra
// row/column per level, so about 2x recomputation at level 0 and less above.  Per pixel the arithmetic
// is that of a plain per-level resize (same tables, same order), so the planes are bit-identical.  The rectangles and the
// table slices are worked out by the host once per frame size (orb_plan; PyrTile, PyrLds and the tile size PT_W x PT_H:
// reloc_orb_plan.h).

// The five ORB kernels of the 1..8 contexts of a call are FIVE launches, blockIdx.y = frame.  Everything a kernel needs of
// one context travels in the kernel arguments (OrbFrame, FrameTable: reloc_internal.h).
template <int N> using OrbFrames = FrameTable<OrbFrame, N>;

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
// The one stage that keeps a pointer-argument kernel for one frame beside its frame-table kernel: the body reads its tables
// (tab, tiles, rz: uniform addresses) between barriers, and only `const __restrict__` kernel arguments let the compiler keep
// those reads scalar -- from a frame table they become ~100 vector loads and the kernel 1.7 us longer (measured: DESIGN.md
// section 4).
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
__global__ __launch_bounds__(PYR_BS) void k_pyramid_batch(OrbFrames<RELOC_BATCH_MAX> b, int w, int h, int sstride, int order_rgb, PyrLds lds)
{
    RELOC_SMALL_KERNEL_PRIO();
    const OrbFrame &F = b.at(blockIdx.y);
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
    __device__ __forceinline__ FastQuad(const u32 (&rows)[7][3], int thr) : w(rows)
    {
        const u32 c = rows[3][1];
        const u32 ce = c & 0x00FF00FFu, co = (c >> 8) & 0x00FF00FFu;
        // v > c + t  <=>  v + (0x7FFF - c - t) has bit 15;   v < c - t  <=>  (c - t - 1 + 0x8000) - v has bit 15
        // (1 <= t <= 254: neither half borrows from or carries into the other)
        const u32 t2 = (0x7FFFu - (u32)thr) * 0x00010001u;
        nb[0] = t2 - ce; nb[1] = t2 - co;
        nd[0] = t2 + ce; nd[1] = t2 + co;
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

constexpr int FT_P = FT / 4 + 3;       // dwords per staged row: columns x0 - 4 .. x0 + FT + 3, one of padding
static_assert(FT == 32, "fast_nms_tile maps 256 lanes to 32 rows x 8 dwords");
// MASKED: a kept corner whose byte of the mask pyramid (`mask`, geometry of pyr) is 0 enters neither the NMS map nor the
// histogram (include/reloc_spec.h "ORB MASK"); the unmasked instantiation never reads `mask`.
// THR: the FAST threshold as a compile-time constant (the default, RELOC_FAST_THRESHOLD), or 0: the wave-uniform value of the
// table (include/reloc_spec.h "ORB PARAMS").  The host picks the instantiation (orb_run).
template <bool MASKED, int THR>
__device__ __forceinline__ void fast_nms_tile(const OrbTable *__restrict__ tab, const uint8_t *__restrict__ pyr,
                                              uint8_t *__restrict__ nms, int32_t *__restrict__ hist, int bid,
                                              const uint8_t *__restrict__ mask)
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
    const int thr = THR ? THR : tab->fast_thr;
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
        const FastQuad Q(w, thr);
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
            const int nb = (v0 > thr) + (v4 > thr) + (v8 > thr) + (v12 > thr);
            const int nd = (v0 < -thr) + (v4 < -thr) + (v8 < -thr) + (v12 < -thr);
            cand = nb >= 2 || nd >= 2;
        }
        if (tid < 3 * 64 && __any(cand)) {
            if (cand) pol = fast_is_corner(pc, IS, thr);
        }
        if (pol) s_corner[atomicAdd(&s_nc, 1)] = (unsigned short)((ry << 6) | rx | (pol < 0 ? 0x8000 : 0));
    }
    __syncthreads();
    for (int i = tid; i < s_nc; i += 256) {
        const int e16 = s_corner[i], ry = (e16 >> 6) & 63, rx = e16 & 63;
        s_sc[ry * SS + rx] = (uint8_t)fast_corner_score(s_img + (ry + 3) * IS + (rx + 3), IS, thr, (e16 & 0x8000) ? -1 : 1);
    }
    __syncthreads();
    {
        const int ry = tid / 8, rx4 = (tid % 8) * 4;
        u32 word = 0;
        u32 keep = 0;       // MASKED: the mask bytes of the lane's four pixels, one aligned dword
        if constexpr (MASKED)
            if (y0 + ry < L.h) keep = *reinterpret_cast<const u32 *>(mask + L.off + (size_t)(y0 + ry) * L.stride + x0 + rx4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int gx = x0 + rx4 + k, gy = y0 + ry;
            const uint8_t *s = s_sc + (ry + 1) * SS + (rx4 + k + 1);
            const int c = (!MASKED || ((keep >> (8 * k)) & 0xFF)) ? s[0] : 0;
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
// FAST + NMS tiles and 7x7 blur tiles of all levels in ONE launch, one workgroup per tile: both only read the pyramid, FAST
// feeds Harris and the blur feeds the descriptors, so they need not run one after the other.  (A smaller grid whose workgroups
// walk the tiles paid beside 112-register scans and pays nothing beside 104-register ones: profiles/README.md "Dropped
// experiments" #8.)
// MASKED = true: the same with the detection mask applied behind NMS; the frame's `mask` is unread otherwise.
// THR: fast_nms_tile.
template <bool MASKED, int THR, int N>
__global__ __launch_bounds__(256) void k_fast_blur(OrbFrames<N> b, int n_fast)
{
    RELOC_SMALL_KERNEL_PRIO();
    const OrbFrame &F = b.at(blockIdx.y);
    if ((int)blockIdx.x < n_fast) fast_nms_tile<MASKED, THR>(F.tab, F.pyr, F.nms, F.hist, (int)blockIdx.x, F.mask);
    else blur7_tile(F.tab, F.pyr, F.blur, (int)blockIdx.x - n_fast);
}

// ---- mask pyramid -------------------------------------------------------------------------------
// Level l of a mask pyramid from its level l - 1 (include/reloc_spec.h "ORB MASK"): the image pyramid's resize (same table
// slices, same arithmetic), then THRESH_TOZERO.  A lane writes the four pixels of one dword, the row padding as 0; one launch
// per level, each reading what the one before wrote.  Runs when a mask is set, not per frame.
__global__ __launch_bounds__(256) void k_mask_level(const OrbTable *__restrict__ tab, const int32_t *__restrict__ rz,
                                                    uint8_t *__restrict__ mp, int l)
{
    const OrbLevel S = tab->lev[l - 1], D = tab->lev[l];
    const int x4 = 4 * (int)(blockIdx.x * 256 + threadIdx.x), y = (int)blockIdx.y;
    if (x4 >= D.stride || y >= D.h) return;
    const int32_t *xo = rz + tab->rz_off[l][0], *xc = rz + tab->rz_off[l][1];
    const int sy0 = rz[tab->rz_off[l][2] + y], sy1 = sy0 + 1 < S.h ? sy0 + 1 : S.h - 1;
    const u32 b = (u32)rz[tab->rz_off[l][3] + y], one = 1u << RELOC_RESIZE_COEF_BITS;
    const uint8_t *r0 = mp + S.off + (size_t)sy0 * S.stride, *r1 = mp + S.off + (size_t)sy1 * S.stride;
    u32 out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (x4 + k < D.w) {
            const int k0 = xo[x4 + k], k1 = k0 + 1 < S.w ? k0 + 1 : S.w - 1;
            const u32 a = (u32)xc[x4 + k];
            const u32 h0 = (u32)r0[k0] * (one - a) + (u32)r0[k1] * a;
            const u32 h1 = (u32)r1[k0] * (one - a) + (u32)r1[k1] * a;
            const u32 v = (h0 * (one - b) + h1 * b + (1u << 15)) >> 16;
            if (v > RELOC_ORB_MASK_THRESH) out |= v << (8 * k);
        }
    }
    *reinterpret_cast<u32 *>(mp + D.off + (size_t)y * D.stride + x4) = out;
}

// cut score from the level's histogram (KeyPointsFilter::retainBest(n_keep) with ties kept, raised
// while the kept set exceeds RELOC_ORB_STAGE1_CAP), by ONE wave without block barriers: lane i owns the
// bins 4i .. 4i+3.  c(s) = sum_{k >= s} hist[k] is non-increasing in s;
//   cut0 = max{s : c(s) >= n_keep} if c(0) > n_keep, else the FAST threshold in use, thr (everything is kept);
//   cut  = min{s >= cut0 : c(s) <= CAP or s == 255}.
// Every lane returns the cut.
__device__ int stage1_cut_wave(const int32_t *__restrict__ hist_l, int n_keep, int lane, int thr)
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
    int cut0 = thr;
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
// MODE (include/reloc_spec.h "ORB PARAMS"; the host picks, orb_run): ORB_MODE_DEFAULT = the default threshold as a constant,
// Harris score; ORB_MODE_HARRIS = the table's threshold; ORB_MODE_FAST = the table's threshold, n_keep = quota, and the
// survivors enter the candidate list with their FAST score as the response: no Harris sums.
enum { ORB_MODE_DEFAULT = 0, ORB_MODE_HARRIS = 1, ORB_MODE_FAST = 2 };
template <int MODE>
__device__ __forceinline__ void harris_body(const OrbTable *__restrict__ tab, const uint8_t *__restrict__ pyr,
                                                const uint8_t *__restrict__ nms, const int32_t *__restrict__ hist,
                                                int32_t *__restrict__ cand_cnt, u32 *__restrict__ cand_key,
                                                float *__restrict__ cand_resp, int32_t *__restrict__ dbg_cut)
{
    __shared__ int s_cut;
    __shared__ int s_n, s_base;
    __shared__ u32 s_list[HARRIS_CHUNK];
    const int thr = MODE == ORB_MODE_DEFAULT ? RELOC_FAST_THRESHOLD : tab->fast_thr;
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
        const int c = stage1_cut_wave(hist + l * 256, MODE == ORB_MODE_FAST ? L.quota : 2 * L.quota, threadIdx.x, thr);
        if (threadIdx.x == 0) {
            s_cut = c;
            if (dbg_cut) dbg_cut[l] = c;
        }
    }
    __syncthreads();
    const int cut = s_cut;
    if constexpr (MODE == ORB_MODE_FAST) {
        // every survivor is a candidate: the lane that found it files it, one slot reservation per survivor
        if (any) {
#pragma unroll
            for (int k = 0; k < HARRIS_CHUNK / 256; ++k) {
                const int sc = (v >> (8 * k)) & 0xFF;
                if (sc && sc >= cut) {
                    const int64_t idx = idx0 + k;
                    const int y = (int)(idx / L.stride), x = (int)(idx % L.stride);
                    const int pos = atomicAdd(&cand_cnt[l], 1);
                    if (pos < RELOC_ORB_STAGE1_CAP) {
                        cand_key[(size_t)l * RELOC_ORB_STAGE1_CAP + pos] = ((u32)y << 16) | (u32)x;
                        cand_resp[(size_t)l * RELOC_ORB_STAGE1_CAP + pos] = (float)sc;
                    }
                }
            }
        }
        return;
    }
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
template <int MODE, int N>
__global__ __launch_bounds__(256) void k_harris(OrbFrames<N> b)
{
    RELOC_SMALL_KERNEL_PRIO();
    const OrbFrame &F = b.at(blockIdx.y);
    harris_body<MODE>(F.tab, F.pyr, F.nms, F.hist, F.cand_cnt, F.cand_key, F.cand_resp, F.dbg_cut);
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
template <int N>
__global__ __launch_bounds__(1024) void k_select(OrbFrames<N> b)
{
    RELOC_SMALL_KERNEL_PRIO();
    const OrbFrame &F = b.at(blockIdx.y);
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
template <int N>
__global__ __launch_bounds__(256) void k_describe(OrbFrames<N> b, int max_feat)
{
    RELOC_SMALL_KERNEL_PRIO();
    const OrbFrame &F = b.at(blockIdx.y);
    describe_body(F.tab, F.pyr, F.blur, F.kp_cnt, F.kp_key, F.kp_resp, max_feat, F.f_xy, F.f_size, F.f_angle, F.f_resp, F.f_oct, F.f_desc,
                  F.f_count);
}

// ------------------------------------------------------------------------------------------------
// The three pyramid arenas, and both mask pyramids (level 0 of the persistent one first: `keep` bytes of it survive a growth),
// of pyr_bytes each
static int orb_arenas_layout(reloc_ctx *ctx, int64_t pyr_bytes)
{
    OrbFrame &b = ctx->orb.buf;
    return ctx->orb.arenas.layout(ctx, [&](BlockCarver &c) { for (uint8_t **p : {&b.pyr, &b.blur, &b.nms}) c.own(*p, pyr_bytes); });
}
static int orb_mask_layout(reloc_ctx *ctx, int64_t pyr_bytes, size_t keep)
{
    OrbMaskStage &m = ctx->orb.mask;
    return m.block.layout(ctx, [&](BlockCarver &c) { c.own(m.pyr, pyr_bytes); c.own(m.call, pyr_bytes); }, keep);
}

// The fixed blocks of a context's ORB state, sized for its capacity (orb_caps) and its feature rows
int orb_alloc(reloc_ctx *ctx)
{
    OrbState &o = ctx->orb;
    OrbFrame &b = o.buf;
    const int64_t mf = ctx->max_feat, s1 = (int64_t)NLEV * RELOC_ORB_STAGE1_CAP;
    o.caps = orb_caps(ctx->max_w, ctx->max_h);
    if (int rc = orb_arenas_layout(ctx, o.caps.pyr_bytes)) return rc;
    return o.fixed.layout(ctx, [&](BlockCarver &c) {
        c.own(b.tab, 1);
        c.own(b.rz, o.caps.rz_entries);
        c.own(b.tiles, o.caps.tiles);
        c.own(b.hist, NLEV * 256);
        for (int32_t **p : {&b.cand_cnt, &b.kp_cnt, &b.dbg_cut}) c.own(*p, NLEV);
        for (uint32_t **p : {&b.cand_key, &b.kp_key}) c.own(*p, s1);
        for (float **p : {&b.cand_resp, &b.kp_resp}) c.own(*p, s1);
        c.own(b.f_xy, mf * 2);
        for (float **p : {&b.f_size, &b.f_angle, &b.f_resp}) c.own(*p, mf);
        c.own(b.f_oct, mf);
        c.own(b.f_desc, mf * 32);
        c.own(b.f_count, 1);
    });
}

// The blocks whose size depends on the ORB parameters (the three pyramid arenas, both mask pyramids) grown for prm when the
// context holds less; they never shrink, and a context that keeps the defaults keeps what orb_alloc took.  The arenas hold
// nothing that outlives a frame except level 0 of the persistent mask, which moves.
static int orb_grow(reloc_ctx *ctx, const OrbParams &prm)
{
    OrbState &o = ctx->orb;
    const OrbCaps want = orb_caps(ctx->max_w, ctx->max_h, prm);
    if (want.pyr_bytes <= o.caps.pyr_bytes) return RELOC_OK;
    OrbMaskStage &m = o.mask;
    if (m.pyr) {      // the mask block first: if the arenas fail behind it, it is only larger than it need be
        const size_t level0 = m.on() ? (size_t)((m.w + 63) / 64 * 64) * m.h : 0;
        if (int rc = orb_mask_layout(ctx, want.pyr_bytes, level0)) return rc;
        m.built = false;
        m.last = nullptr;
    }
    if (int rc = orb_arenas_layout(ctx, want.pyr_bytes)) return rc;
    o.caps.pyr_bytes = want.pyr_bytes;
    o.w = o.h = o.nfeat = 0;      // the debug planes of the last frame went with the old arenas
    return RELOC_OK;
}

static bool g_pattern_uploaded[64] = {};

// Capacity check, cache hit, plan, then the three tables go to the device with the cache key taken down: a failed upload
// leaves a context without geometry (the next frame plans again), never one whose key names tables that were half replaced.
int orb_prepare(reloc_ctx *ctx, int w, int h, int nfeatures, const OrbParams &prm)
{
    OrbState &o = ctx->orb;
    if (w > ctx->max_w || h > ctx->max_h) {
        reloc_set_error("frame %dx%d exceeds the ctx capacity %dx%d", w, h, ctx->max_w, ctx->max_h);
        return RELOC_E_CAPACITY;
    }
    if (o.w == w && o.h == h && o.nfeat == nfeatures && o.plan_prm.same(prm)) return RELOC_OK;
    if (!g_pattern_uploaded[ctx->device & 63]) {
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_pattern), RELOC_ORB_PATTERN, sizeof(RELOC_ORB_PATTERN)));
        g_pattern_uploaded[ctx->device & 63] = true;
    }
    const OrbPlan plan = orb_plan(w, h, nfeatures, o.caps, prm);
    if (plan.rc) { reloc_set_error("%s", plan.err); return plan.rc; }
    o.w = o.h = o.nfeat = 0;
    const hipError_t e0 = hipMemcpyAsync(const_cast<PyrTile *>(o.buf.tiles), plan.tiles.data(), sizeof(PyrTile) * plan.tiles.size(),
                                         hipMemcpyHostToDevice, ctx->stream);
    const hipError_t e1 = hipMemcpyAsync(const_cast<int32_t *>(o.buf.rz), plan.rz.data(), sizeof(int32_t) * plan.rz.size(),
                                         hipMemcpyHostToDevice, ctx->stream);
    const hipError_t e2 = hipMemcpyAsync(const_cast<OrbTable *>(o.buf.tab), &plan.tab, sizeof(OrbTable), hipMemcpyHostToDevice, ctx->stream);
    const hipError_t e3 = hipStreamSynchronize(ctx->stream);      // the plan's arrays leave with this function
    HIP_TRY(e0); HIP_TRY(e1); HIP_TRY(e2); HIP_TRY(e3);
    memcpy(&o.tab, &plan.tab, sizeof(OrbTable));
    o.lds = plan.lds; o.lds_bytes = plan.lds_bytes; o.ntiles = (int)plan.tiles.size();
    o.w = w; o.h = h; o.nfeat = nfeatures; o.plan_prm = prm;
    return RELOC_OK;
}

// first use of a mask: both mask pyramids as one block
static int mask_alloc(reloc_ctx *ctx)
{
    OrbMaskStage &m = ctx->orb.mask;
    return m.pyr ? (int)RELOC_OK : orb_mask_layout(ctx, ctx->orb.caps.pyr_bytes, 0);
}

// levels 1.. of the mask pyramid mp of a prepared context from its level 0, on the context's stream
static void mask_pyramid_launch(reloc_ctx *c, uint8_t *mp)
{
    for (int l = 1; l < NLEV; ++l) {
        const OrbLevel &L = c->orb.tab.lev[l];
        if (L.w < 1 || L.h < 1) break;
        hipLaunchKernelGGL(k_mask_level, dim3((L.stride / 4 + 255) / 256, L.h), dim3(256), 0, c->stream, c->orb.buf.tab, c->orb.buf.rz, mp, l);
    }
}

// Five launches behind the image chain (reloc_image.hip): the frames are of equal geometry.  The chain serves the frames
// of the entry points (chain: 3-channel, raw mosaics with the Bayer stage on, or the contexts' pixel format), never a
// caller's gray plane (!chain); with the downscale
// stage on, w x h is the source size and everything from orb_prepare on sees the working frame.  The pyramid reads the last
// plane the chain wrote, or the frame itself.  It runs 512-thread workgroups for latency, 256 where it shares the chip with
// whole-database scans.
template <int N>
static void orb_launch(reloc_ctx *c0, int n, const OrbFrames<RELOC_BATCH_MAX> &all, const OrbParams &P, int w, int h, int stride,
                       int flags, int channels, bool aligned, bool masked, bool latency)
{
    const OrbFrames<N> b = frame_table<N>(all);
    const OrbTable *tab_h = &c0->orb.tab;
    hipStream_t st = c0->stream;
    const int n_fast = tab_h->fast_tile_base[NLEV], n_blur = tab_h->blur_tile_base[NLEV];
    // the default detector runs the kernels built for it; any other threshold or score the ones that read the table
    const bool thr_def = P.fast_thr == RELOC_FAST_THRESHOLD;
    const int mode = P.score == RELOC_ORB_FAST_SCORE ? ORB_MODE_FAST : thr_def ? ORB_MODE_DEFAULT : ORB_MODE_HARRIS;
    if constexpr (N == 1) {         // k_pyramid: pointer arguments for one frame, and only one frame gets the 512-thread shape
        const OrbFrame &F = b.f[0];
        auto kern512 = channels == 3 ? (aligned ? k_pyramid<3, true, 512> : k_pyramid<3, false, 512>) : (aligned ? k_pyramid<1, true, 512> : k_pyramid<1, false, 512>);
        auto kern256 = channels == 3 ? (aligned ? k_pyramid<3, true, 256> : k_pyramid<3, false, 256>) : (aligned ? k_pyramid<1, true, 256> : k_pyramid<1, false, 256>);
        hipLaunchKernelGGL(latency ? kern512 : kern256, dim3(c0->orb.ntiles), dim3(latency ? 512 : 256), c0->orb.lds_bytes, st, F.tab,
                           F.tiles, F.rz, F.src, w, h, stride, flags, F.pyr, c0->orb.lds, F.hist, F.cand_cnt);
    } else {
        auto kern = channels == 3 ? (aligned ? k_pyramid_batch<3, true, 256> : k_pyramid_batch<3, false, 256>)
                                  : (aligned ? k_pyramid_batch<1, true, 256> : k_pyramid_batch<1, false, 256>);
        hipLaunchKernelGGL(kern, dim3(c0->orb.ntiles, n), dim3(256), c0->orb.lds_bytes, st, b, w, h, stride, flags, c0->orb.lds);
    }
    auto fast = masked ? (thr_def ? k_fast_blur<true, RELOC_FAST_THRESHOLD, N> : k_fast_blur<true, 0, N>)
                       : (thr_def ? k_fast_blur<false, RELOC_FAST_THRESHOLD, N> : k_fast_blur<false, 0, N>);
    auto harris = mode == ORB_MODE_FAST ? k_harris<ORB_MODE_FAST, N>
                                        : mode == ORB_MODE_HARRIS ? k_harris<ORB_MODE_HARRIS, N> : k_harris<ORB_MODE_DEFAULT, N>;
    hipLaunchKernelGGL(fast, dim3(n_fast + n_blur, n), dim3(256), 0, st, b, n_fast);
    hipLaunchKernelGGL(harris, dim3(tab_h->flat_base[NLEV], n), dim3(256), 0, st, b);
    hipLaunchKernelGGL(k_select<N>, dim3(NLEV, n), dim3(1024), 0, st, b);
    hipLaunchKernelGGL(k_describe<N>, dim3((c0->max_feat + 3) / 4, n), dim3(256), 0, st, b, c0->max_feat);
}

int orb_run(reloc_ctx *const *ctxs, int n, const uint8_t *const *srcs, int w, int h, int stride, bool chain, int order,
            int nfeatures, bool latency, bool call_mask, const OrbParams *call_prm)
{
    if (n < 1 || n > RELOC_BATCH_MAX) { reloc_set_error("orb: 1..%d frames", RELOC_BATCH_MAX); return RELOC_E_ARG; }
    reloc_ctx *c0 = ctxs[0];
    const OrbParams P = call_prm ? *call_prm : c0->orb.prm;
    const int sw = w, sh = h;               // the frame as handed in; w x h becomes the working frame
    if (int rc = image_chain_check(ctxs, n, chain, &w, &h)) return rc;
    for (int f = 0; f < n; ++f) {
        reloc_ctx *c = ctxs[f];
        if (!call_prm && !c->orb.prm.same(P)) {
            reloc_set_error("orb batch: contexts with unequal ORB parameters (reloc_set_orb_params)");
            return RELOC_E_STATE;
        }
        if (int rc = orb_prepare(c, w, h, nfeatures, P)) return rc;
        if (c->orb.ntiles != c0->orb.ntiles || c->orb.lds_bytes != c0->orb.lds_bytes || c->max_feat != c0->max_feat ||
            c->prm.gray_coeff_bits != c0->prm.gray_coeff_bits) {
            reloc_set_error("orb batch: contexts of unequal geometry");
            return RELOC_E_STATE;
        }
        if (int rc = image_chain_check_prepared(ctxs, f, n, chain, w, h)) return rc;
        if (chain && !c->orb.mask.same(c0->orb.mask)) {
            reloc_set_error("orb batch: contexts with and without a detection mask, or with masks of unequal size (reloc_set_orb_mask)");
            return RELOC_E_STATE;
        }
    }
    // the persistent mask serves the frames of the chain and has the size of their working frame; nothing is launched otherwise
    const bool masked = call_mask || (chain && c0->orb.mask.on());
    if (masked && !call_mask && (w != c0->orb.mask.w || h != c0->orb.mask.h)) {
        reloc_set_error("working frame %dx%d differs from the detection mask %dx%d (reloc_set_orb_mask)", w, h, c0->orb.mask.w, c0->orb.mask.h);
        return RELOC_E_ARG;
    }
    if (masked)
        for (int f = 0; f < n; ++f) {
            OrbMaskStage &m = ctxs[f]->orb.mask;
            if (call_mask) mask_pyramid_launch(ctxs[f], m.call);
            else if (!m.built || !m.built_prm.same(P)) { mask_pyramid_launch(ctxs[f], m.pyr); m.built = true; m.built_prm = P; }
            m.last = call_mask ? m.call : m.pyr; m.last_w = w; m.last_h = h;
        }
    const int flags = gray_flags(c0, order);
    reloc_prof_begin(c0, RELOC_PROF_ORB);
    const uint8_t *planes[RELOC_BATCH_MAX];
    int channels = 1;       // of what the pyramid reads: the last plane the chain wrote, a gray plane, or a 3-channel frame
    if (int rc = image_chain_gray(ctxs, n, chain, &srcs, sw, sh, w, h, &stride, &channels, flags, planes)) {
        reloc_prof_end(c0, RELOC_PROF_ORB);
        return rc;
    }
    bool aligned = w % 4 == 0 && stride % 4 == 0;
    for (int f = 0; f < n; ++f) aligned = aligned && ((uintptr_t)srcs[f]) % 4 == 0;
    OrbFrames<RELOC_BATCH_MAX> b;
    frame_slots(ctxs, n, [&](int f, reloc_ctx *c, int g) { b.f[f] = c->orb.buf; b.f[f].src = srcs[g]; b.f[f].mask = masked ? c->orb.mask.last : nullptr; });
    n == 1 ? orb_launch<1>(c0, n, b, P, w, h, stride, flags, channels, aligned, masked, latency)
           : orb_launch<RELOC_BATCH_MAX>(c0, n, b, P, w, h, stride, flags, channels, aligned, masked, latency);
    reloc_prof_end(c0, RELOC_PROF_ORB);
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

RELOC_API int reloc_orb_frame_dev(reloc_ctx *ctx, const uint8_t *img_dev, int w, int h, int stride, int order, int nfeatures)
{
    ARG_CHECK_CTX(ctx, img_dev && w >= 64 && h >= 64 && nfeatures > 0, "reloc_orb_frame_dev");
    ARG_CHECK(stride >= w * image_chain_frame_bpp(ctx), "reloc_orb_frame_dev");
    return orb_run(&ctx, 1, &img_dev, w, h, stride, true, order, nfeatures, true);
}

RELOC_API const uint8_t *reloc_frame_desc_dev(reloc_ctx *ctx) { return ctx ? ctx->orb.buf.f_desc : nullptr; }
RELOC_API const float *reloc_frame_xy_dev(reloc_ctx *ctx) { return ctx ? ctx->orb.buf.f_xy : nullptr; }
RELOC_API const int32_t *reloc_frame_count_dev(reloc_ctx *ctx) { return ctx ? ctx->orb.buf.f_count : nullptr; }

// level 0 of the mask pyramid mp from a host mask of w x h (rows mask_stride apart): rows of the level's stride, padding 0
static int mask_upload(reloc_ctx *ctx, uint8_t *mp, const uint8_t *mask, int w, int h, int mask_stride)
{
    const size_t ds = (size_t)((w + 63) / 64 * 64);
    HIP_TRY(hipMemsetAsync(mp, 0, ds * h, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(mp, ds, mask, mask_stride, w, h, hipMemcpyHostToDevice, ctx->stream));
    return RELOC_OK;
}

// gray plane -> features on the host; mask != NULL: under that mask, through the context's per-call mask pyramid;
// prm != NULL: with these ORB parameters for this call, the persistent ones untouched
static int orb_detect_host(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride, const uint8_t *mask, int mask_stride,
                           const OrbParams *prm, int nfeatures, float *xy, float *size, float *angle, float *response,
                           int32_t *octave, uint8_t *desc, int32_t *n_out)
{
    *n_out = 0;
    if (w < 63 || h < 63) return RELOC_OK;   // no level is wider than the 31-pixel edge margin on both sides
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    if (prm)
        if (int rc = orb_grow(ctx, *prm)) return rc;
    if (mask)
        if (int rc = mask_alloc(ctx)) return rc;
    HostStaging st{ctx};        // no scratch slot: the context's frame and feature buffers
    st.upload_rows(ctx->frame_img, gray, w, h, stride);
    if (mask) st.run([&] { return mask_upload(ctx, ctx->orb.mask.call, mask, w, h, mask_stride); });
    const uint8_t *src = ctx->frame_img;
    st.run([&] { return orb_run(&ctx, 1, &src, w, h, w, false, 0, nfeatures, true, mask != nullptr, prm); });
    const int32_t n = st.count(ctx->orb.buf.f_count);
    if (n > 0) {
        if (xy) st.download(xy, ctx->orb.buf.f_xy, (int64_t)n * 8);
        if (size) st.download(size, ctx->orb.buf.f_size, (int64_t)n * 4);
        if (angle) st.download(angle, ctx->orb.buf.f_angle, (int64_t)n * 4);
        if (response) st.download(response, ctx->orb.buf.f_resp, (int64_t)n * 4);
        if (octave) st.download(octave, ctx->orb.buf.f_oct, (int64_t)n * 4);
        if (desc) st.download(desc, ctx->orb.buf.f_desc, (int64_t)n * 32);
    }
    if (int rc = st.finish()) return rc;
    *n_out = n;
    return RELOC_OK;
}

RELOC_API int reloc_orb_detect_compute(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride, int nfeatures,
                                       float *xy, float *size, float *angle, float *response, int32_t *octave,
                                       uint8_t *desc, int32_t *n_out)
{
    ARG_CHECK_CTX(ctx, gray && n_out && w > 0 && h > 0 && stride >= w && nfeatures > 0, "reloc_orb_detect_compute");
    return orb_detect_host(ctx, gray, w, h, stride, nullptr, 0, nullptr, nfeatures, xy, size, angle, response, octave, desc, n_out);
}

RELOC_API int reloc_orb_detect_compute_masked(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride, const uint8_t *mask,
                                              int mask_stride, int nfeatures, float *xy, float *size, float *angle,
                                              float *response, int32_t *octave, uint8_t *desc, int32_t *n_out)
{
    ARG_CHECK_CTX(ctx, gray && n_out && w > 0 && h > 0 && stride >= w && nfeatures > 0, "reloc_orb_detect_compute_masked");
    ARG_CHECK(mask && mask_stride >= w, "reloc_orb_detect_compute_masked: mask is NULL or its stride is below the width");
    return orb_detect_host(ctx, gray, w, h, stride, mask, mask_stride, nullptr, nfeatures, xy, size, angle, response, octave, desc, n_out);
}

static int orb_params_check(const OrbParams &p, const char *who)
{
    if (const char *bad = p.check()) { reloc_set_error("bad argument: %s: %s", who, bad); return RELOC_E_ARG; }
    return RELOC_OK;
}

RELOC_API int reloc_orb_detect_compute_params(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride, const uint8_t *mask,
                                              int mask_stride, int nfeatures, int nlevels, double scale_factor, int fast_threshold,
                                              int score_type, float *xy, float *size, float *angle, float *response,
                                              int32_t *octave, uint8_t *desc, int32_t *n_out)
{
    ARG_CHECK_CTX(ctx, gray && n_out && w > 0 && h > 0 && stride >= w && nfeatures > 0, "reloc_orb_detect_compute_params");
    ARG_CHECK(!mask || mask_stride >= w, "reloc_orb_detect_compute_params: the mask's stride is below the width");
    const OrbParams prm{nlevels, scale_factor, fast_threshold, score_type};
    if (int rc = orb_params_check(prm, "reloc_orb_detect_compute_params")) return rc;
    return orb_detect_host(ctx, gray, w, h, stride, mask, mask_stride, &prm, nfeatures, xy, size, angle, response, octave, desc, n_out);
}

RELOC_API int reloc_set_orb_params(reloc_ctx *ctx, int nlevels, double scale_factor, int fast_threshold, int score_type)
{
    ARG_CHECK_CTX(ctx, true, "ctx is NULL");
    const OrbParams prm{nlevels, scale_factor, fast_threshold, score_type};
    if (int rc = orb_params_check(prm, "reloc_set_orb_params")) return rc;
    if (int rc = orb_grow(ctx, prm)) return rc;
    ctx->orb.prm = prm;
    return RELOC_OK;
}

RELOC_API int reloc_get_orb_params(reloc_ctx *ctx, int32_t *nlevels, double *scale_factor, int32_t *fast_threshold, int32_t *score_type)
{
    ARG_CHECK_CTX(ctx, nlevels && scale_factor && fast_threshold && score_type, "reloc_get_orb_params");
    const OrbParams &p = ctx->orb.prm;
    *nlevels = p.nlevels; *scale_factor = p.scale; *fast_threshold = p.fast_thr; *score_type = p.score;
    return RELOC_OK;
}

RELOC_API int reloc_set_orb_mask(reloc_ctx *ctx, const uint8_t *mask, int w, int h, int stride)
{
    ARG_CHECK_CTX(ctx, true, "ctx is NULL");
    OrbMaskStage &m = ctx->orb.mask;
    if (!mask || (w == 0 && h == 0)) {
        m.w = m.h = 0;
        m.built = false;
        return RELOC_OK;
    }
    ARG_CHECK(w >= 1 && h >= 1 && stride >= w, "reloc_set_orb_mask: the size is not positive or the stride is below the width");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("detection mask exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    if (int rc = mask_alloc(ctx)) return rc;
    // frames in flight may still read the previous mask; its levels 1.. are built in front of the next frame, when the
    // tables of the frame size exist
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    m.w = m.h = 0;
    m.built = false;
    if (m.last == m.pyr) m.last = nullptr;      // its levels no longer belong together: no tap until a frame used the new mask
    if (int rc = mask_upload(ctx, m.pyr, mask, w, h, stride)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    m.w = w; m.h = h;
    return RELOC_OK;
}

RELOC_API int reloc_get_orb_mask(reloc_ctx *ctx, int32_t *w, int32_t *h)
{
    ARG_CHECK_CTX(ctx, w && h, "reloc_get_orb_mask");
    *w = ctx->orb.mask.w; *h = ctx->orb.mask.h;
    return RELOC_OK;
}

RELOC_API int reloc_orb_mask_level(reloc_ctx *ctx, int level, uint8_t *out, int32_t *w, int32_t *h)
{
    ARG_CHECK_CTX(ctx, out && w && h && level >= 0 && level < NLEV, "reloc_orb_mask_level");
    const OrbMaskStage &m = ctx->orb.mask;
    if (!m.last || m.last_w != ctx->orb.w || m.last_h != ctx->orb.h) { reloc_set_error("no masked frame processed yet"); return RELOC_E_STATE; }
    const OrbLevel &L = ctx->orb.tab.lev[level];
    if (L.w < 1 || L.h < 1) { *w = *h = 0; return RELOC_OK; }      // a level behind nlevels
    HIP_TRY(hipMemcpy2DAsync(out, L.w, m.last + L.off, L.stride, L.w, L.h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *w = L.w;
    *h = L.h;
    return RELOC_OK;
}

RELOC_API int reloc_frame_debug_plane(reloc_ctx *ctx, int what, int level, uint8_t *out, int32_t *w, int32_t *h)
{
    ARG_CHECK_CTX(ctx, out && w && h && what >= 0 && what <= 2 && level >= 0 && level < NLEV, "reloc_frame_debug_plane");
    if (!ctx->orb.w) { reloc_set_error("no frame processed yet"); return RELOC_E_STATE; }
    const OrbLevel &L = ctx->orb.tab.lev[level];
    if (L.w < 1 || L.h < 1) { *w = *h = 0; return RELOC_OK; }      // a level behind nlevels
    const uint8_t *src = (what == 0 ? ctx->orb.buf.pyr : what == 1 ? ctx->orb.buf.blur : ctx->orb.buf.nms) + L.off;
    HIP_TRY(hipMemcpy2DAsync(out, L.w, src, L.stride, L.w, L.h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *w = L.w;
    *h = L.h;
    return RELOC_OK;
}

// The stage record of the last frame, read only: nothing in a frame's launches exists for it.  dbg_cut keeps the cut of an
// earlier frame where no block of this one reached the cut computation, which is the case exactly when the level's
// histogram sums to 0 (no NMS survivor in any chunk): those levels report -1.
RELOC_API int reloc_orb_debug_levels(reloc_ctx *ctx, int32_t *cut, int32_t *cand_cnt, int32_t *kp_cnt)
{
    ARG_CHECK_CTX(ctx, cut && cand_cnt && kp_cnt, "reloc_orb_debug_levels");
    if (!ctx->orb.w) { reloc_set_error("no frame processed yet"); return RELOC_E_STATE; }
    const OrbFrame &b = ctx->orb.buf;
    std::vector<int32_t> hist(NLEV * 256);
    const hipError_t e0 = hipMemcpyAsync(hist.data(), b.hist, sizeof(int32_t) * hist.size(), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e1 = hipMemcpyAsync(cut, b.dbg_cut, sizeof(int32_t) * NLEV, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = hipMemcpyAsync(cand_cnt, b.cand_cnt, sizeof(int32_t) * NLEV, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e3 = hipMemcpyAsync(kp_cnt, b.kp_cnt, sizeof(int32_t) * NLEV, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e4 = hipStreamSynchronize(ctx->stream);      // the histogram copy leaves with this function
    HIP_TRY(e0); HIP_TRY(e1); HIP_TRY(e2); HIP_TRY(e3); HIP_TRY(e4);
    for (int l = 0; l < NLEV; ++l) {
        int64_t sum = 0;
        for (int s = 0; s < 256; ++s) sum += hist[l * 256 + s];
        if (sum == 0) cut[l] = -1;
    }
    return RELOC_OK;
}
