// reloc_stereo_dense.hip -- dense stereo depth on gfx950 (include/reloc_spec.h, "STEREO, dense"): the specification of
// reloc_stereo.hip's sparse matcher at every integer pixel, with the optional semi-global aggregation between costs and
// selection (second half of this file; "STEREO, semi-global").  The decision per pixel is reloc_stereo_match.h's.
//   k_stereo_dense<NP, VOL, COST>  (COST: SAD over gray planes, or the Hamming distance over the census planes of
//                          reloc_census.hip -- "STEREO, census"; only the column cost differs)
//                          a workgroup of four waves takes DT_W output columns of one row, a wave 64 of them; lanes over
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
#include "reloc_stereo_match.h"

constexpr int DT_W = 256;                                   // output columns of a workgroup
constexpr int DT_L = DT_W + 2 * SR;                         // staged columns of the left eye
constexpr int DT_R = DT_L + RELOC_STEREO_NUM_DISP_MAX;      // ... of the right eye, and words of the right map's piece
constexpr uint16_t SGM_NONE = 0xFFFFu;   // an entry of the semi-global cost volume outside D(u): above every SAD (30 855) and census cost (968)

// the instantiation of a kernel template <int NP, ...> for np = ceil(num_disparities / 64) in 1 .. STEREO_PASSES
#define STEREO_NP_KERNEL(np, kern, ...) \
    ((np) == 1 ? kern<1, ##__VA_ARGS__> : (np) == 2 ? kern<2, ##__VA_ARGS__> : (np) == 3 ? kern<3, ##__VA_ARGS__> : kern<4, ##__VA_ARGS__>)
static_assert(STEREO_PASSES == 4, "STEREO_NP_KERNEL names every NP");
// ... of k_stereo_dense<NP, vol, COST> for cost = RELOC_STEREO_COST_*
#define STEREO_DENSE_KERNEL(np, vol, cost) \
    ((cost) ? STEREO_NP_KERNEL(np, k_stereo_dense, vol, RELOC_STEREO_COST_CENSUS) : STEREO_NP_KERNEL(np, k_stereo_dense, vol, RELOC_STEREO_COST_SAD))

// the bytes of column x, rows v - R .. v + R, in three dwords (row v - R in the low byte of .x)
__device__ __forceinline__ uint4 stereo_pack_column(const uint8_t *__restrict__ img, int stride, int v, int x)
{
    const uint8_t *p = img + (size_t)(v - SR) * stride + x;
    uint32_t r[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < SP; ++j) r[j >> 2] |= (uint32_t)p[(size_t)j * stride] << (8 * (j & 3));
    return make_uint4(r[0], r[1], r[2], 0u);
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

// The frame of the two tile kernels, k_stereo_dense and k_sgm_select: a workgroup of 256 threads takes the DT_W columns from U0
// of row blockIdx.y, wave k the 64 from U0 + 64 k, and keeps its piece of the row's right map in s_dr (DT_R words).
template <int NP>
struct StereoTile {
    int tid, lane, v, U0, U1;
    int ulo, uhi;                 // the workgroup's pixels that pass step 1: ulo <= u < uhi
    int wlo, whi;                 // ... and the wave's
    // staged columns: the left eye's xlo .. xlo + nl - 1 (all inside the row), the right eye's rb .. rb + nr - 1, which the
    // lanes of the last disparities reach; the piece of the right map covers the latter
    int xlo, nl, rb, nr;
    size_t row;

    // false (workgroup-uniform): no pixel of the tile passes step 1 and the workgroup has nothing to do but border()
    __device__ __forceinline__ bool begin(const StereoParams &p, unsigned *s_dr)
    {
        tid = threadIdx.x; lane = tid & 63;
        v = blockIdx.y; U0 = blockIdx.x * DT_W; U1 = min(U0 + DT_W, p.w);
        ulo = max(U0, SR); uhi = min(U1, p.w - SR);
        row = (size_t)v * p.w;
        if (v < SR || v >= p.h - SR || ulo >= uhi) return false;
        xlo = ulo - SR; nl = uhi - ulo + 2 * SR;
        rb = xlo - p.min_disp - 64 * NP + 1; nr = nl + 64 * NP - 1;
        const int S0 = U0 + 64 * __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: the walk's bounds and branches stay scalar
        wlo = max(S0, SR); whi = min(S0 + 64, uhi);
        for (int e = tid; e < nr; e += 256) s_dr[e] = KEY_NONE;          // the caller's barrier stands between this and pixel()
        return true;
    }
    // status BORDER for the tile's pixels that fail step 1: all of a workgroup that is not live, else those within R of the
    // row's ends; thread t has column U0 + t
    __device__ __forceinline__ void border(const StereoParams &p, bool live, uint8_t *__restrict__ o_status) const
    {
        const int u = U0 + tid;
        if (u < U1 && (!live || u < SR || u >= p.w - SR)) o_status[row + u] = RELOC_STEREO_BORDER;
    }
    // Steps 2 to 5 of pixel (u, v) by its wave, cost as stereo_select takes it: status and best by lane 0, and with the
    // left-right check on the keys of the lanes inside D into s_dr at column u - d.
    template <typename Best>
    __device__ __forceinline__ void pixel(const int (&cost)[NP], const StereoParams &p, int u, unsigned *s_dr, Best *__restrict__ o_best,
                                          uint8_t *__restrict__ o_status) const
    {
        const int dmin = p.min_disp, dhi = min(dmin + p.num_disp - 1, u - SR);
        if (p.lr) {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const int d = dmin + 64 * q + lane;
                if (d <= dhi) atomicMin(&s_dr[u - d - rb], stereo_key(cost[q], d));
            }
        }
        const StereoPick s = stereo_select<NP>(cost, dmin, dhi, p.uniq, lane);
        if (lane == 0) {
            o_status[row + u] = (uint8_t)s.status;
            stereo_best_store(o_best + row + u, s.dstar, s.a, s.b, s.c);
        }
    }
    // the workgroup's piece of the row's right map, once every wave has walked: column rb + e; a key exists only where
    // 0 <= R <= rb + e < w
    __device__ __forceinline__ void flush(const unsigned *s_dr, uint32_t *__restrict__ rmap) const
    {
        __syncthreads();
        for (int e = tid; e < nr; e += 256) {
            const unsigned k = s_dr[e];
            if (k != KEY_NONE) atomicMin(&rmap[row + rb + e], k);
        }
    }
};

// the cost of one column of the window, 11 bytes in three dwords each: three v_sad_u8 over gray bytes, or, over census bytes
// ("STEREO, census"), three xors and three v_bcnt with their addend
template <int COST>
__device__ __forceinline__ unsigned stereo_column_cost(const uint4 &lc, const uint4 &rc)
{
    if constexpr (COST == RELOC_STEREO_COST_CENSUS)
        return (unsigned)__builtin_popcount(lc.x ^ rc.x) + (unsigned)__builtin_popcount(lc.y ^ rc.y) + (unsigned)__builtin_popcount(lc.z ^ rc.z);
    else {
        unsigned cs = __builtin_amdgcn_sad_u8(lc.x, rc.x, 0u);
        cs = __builtin_amdgcn_sad_u8(lc.y, rc.y, cs);
        return __builtin_amdgcn_sad_u8(lc.z, rc.z, cs);
    }
}

// VOL: the volume pass of the semi-global matcher -- the same walk, but a pixel's costs go to vol[(v w + u) nd + k], k = d - dmin,
// as uint16 (SGM_NONE beyond d_hi(u)) and nothing else is written: selection, right map and statuses follow from the sums.
// COST: the planes are gray planes (SAD) or census planes; everything but the column cost is the same code.
template <int NP, bool VOL, int COST>
__global__ __launch_bounds__(256) void k_stereo_dense(const uint8_t *__restrict__ left, int lstride, const uint8_t *__restrict__ right,
                                                      int rstride, StereoParams p, uint32_t *__restrict__ rmap,
                                                      uint2 *__restrict__ o_best, uint8_t *__restrict__ o_status,
                                                      uint16_t *__restrict__ vol)
{
    __shared__ uint4 s_l[DT_L];
    __shared__ uint4 s_r[DT_R];
    __shared__ unsigned s_dr[DT_R];
    StereoTile<NP> t;
    const bool live = t.begin(p, s_dr);
    if (!VOL) t.border(p, live, o_status);
    if (!live) return;
    const int tid = t.tid, lane = t.lane, v = t.v, dmin = p.min_disp, xlo = t.xlo;
    // a column left of the image is 0 and is not fetched
    for (int e = tid; e < t.nl; e += 256) s_l[e] = stereo_pack_column(left, lstride, v, xlo + e);
    for (int e = tid; e < t.nr; e += 256) {
        const int x = t.rb + e;
        s_r[e] = x >= 0 ? stereo_pack_column(right, rstride, v, x) : make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();                                                  // the staged columns, and begin()'s reset of s_dr
    const int wlo = t.wlo, whi = t.whi;
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
                        const unsigned cs = stereo_column_cost<COST>(lc, rc);
                        cost[q] += (int)cs - ring[q][k];
                        ring[q][k] = (int)cs;
                    }
                    if (u >= wlo) {
                        // ---- cost[q] = C(d) of d = dmin + 64 q + lane: steps 2-5 of pixel (u, v), or its line of the volume ----
                        if constexpr (VOL) {
                            uint16_t *line = vol + (t.row + u) * (size_t)p.num_disp;
#pragma unroll
                            for (int q = 0; q < NP; ++q)
                                if (64 * q + lane < p.num_disp) line[64 * q + lane] = dmin + 64 * q + lane <= u - SR ? (uint16_t)cost[q] : SGM_NONE;
                        } else t.pixel(cost, p, u, s_dr, o_best, o_status);
                    }
                }
            }
        }
    }
    if (!VOL && p.lr) t.flush(s_dr, rmap);
}

// pixel i of the w x h planes: step 6 from the right map, steps 7 and 8; Best: uint2 (SAD costs) or uint4 (semi-global sums)
template <typename Best>
__global__ __launch_bounds__(256) void k_stereo_dense_finish(StereoParams p, const uint32_t *__restrict__ rmap,
                                                             const Best *__restrict__ best, uint8_t *__restrict__ status,
                                                             uint16_t *__restrict__ o_mm, float *__restrict__ o_disp)
{
    const int64_t n = (int64_t)p.w * p.h, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    StereoDepth z = {status[i], 0, 0.f};
    if (z.status == RELOC_STEREO_OK) {
        int dstar, a, b, c;
        stereo_best_load(best[i], dstar, a, b, c);
        if (p.lr && abs((int)(rmap[i - dstar] & 0x7FFu) - dstar) > 1) z.status = RELOC_STEREO_LR;
        else z = stereo_depth_of(dstar, a, b, c, p.fx, p.baseline);
        if (z.status != RELOC_STEREO_OK) status[i] = (uint8_t)z.status;
    }
    o_mm[i] = z.mm;
    o_disp[i] = z.disp;
}

// the context's dense block, on its first dense call; a failure leaves the context without one
static int stereo_dense_alloc(reloc_ctx *ctx)
{
    StereoState::Dense &d = ctx->stereo.dense;
    if (d.block.p) return RELOC_OK;
    return d.block.layout(ctx, [&](BlockCarver &c) { stereo_dense_lines(c, d, (int64_t)ctx->max_w * ctx->max_h); });
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
//   k_sgm_select<NP>          the tile of k_stereo_dense (StereoTile), a wave over 64 pixels of a row: a pixel's sums (4 nd
//                             bytes) into the registers that held its costs, then the same selection -- two minima, the right map
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
    StereoTile<NP> t;
    const bool live = t.begin(p, s_dr);
    t.border(p, live, o_status);
    if (!live) return;
    __syncthreads();                                                  // begin()'s reset of s_dr, before any wave pushes a key
    const int lane = t.lane, nd = p.num_disp, wlo = t.wlo, whi = t.whi;
    if (wlo < whi) {                                                  // wave-uniform
        const uint32_t *line = sum + (t.row + wlo) * (size_t)nd + lane;
        int cost[NP], next[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) cost[q] = 64 * q + lane < nd ? (int)line[64 * q] : 0;
        for (int u = wlo; u < whi; ++u, line += nd) {
#pragma unroll
            for (int q = 0; q < NP; ++q) next[q] = u + 1 < whi && 64 * q + lane < nd ? (int)line[nd + 64 * q] : 0;
            t.pixel(cost, p, u, s_dr, o_best, o_status);
#pragma unroll
            for (int q = 0; q < NP; ++q) cost[q] = next[q];
        }
    }
    if (p.lr) t.flush(s_dr, rmap);
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

// The dense pass on ctx's stream into ctx's dense planes (dense rows of p.w); the planes of the eyes are device pointers.
// sgm == NULL: k_stereo_dense and k_stereo_dense_finish; else the semi-global pass: the volume, the paths of sgm->mask, the
// selection over the sums and the same finish.  speckle: then the speckle stage with ctx's setting ("STEREO, speckle"), inside
// the same stopwatch bracket.
// cost: RELOC_STEREO_COST_*; with the census both planes go through k_census first, inside the same bracket, and the tile
// kernels read the census planes.
static int stereo_dense_launch(reloc_ctx *ctx, const uint8_t *left, int lstride, const uint8_t *right, int rstride, const StereoParams &p,
                               int cost, bool speckle, const StereoSgm *sgm)
{
    if (sgm)
        if (int rc = stereo_sgm_alloc(ctx, p.w, p.h, p.num_disp)) return rc;
    if (cost)
        if (int rc = stereo_census_alloc(ctx)) return rc;
    StereoState::Dense &d = ctx->stereo.dense;
    StereoState::Sgm &g = ctx->stereo.sgm;
    const int64_t px = (int64_t)p.w * p.h;
    const int np = (p.num_disp + 63) / 64, slot = sgm ? RELOC_PROF_STEREO_SGM : RELOC_PROF_STEREO_DENSE;
    const dim3 tiles((p.w + DT_W - 1) / DT_W, p.h), pixels((unsigned)((px + 255) / 256));
    reloc_prof_begin(ctx, slot);
    hipError_t reset = sgm ? hipMemsetAsync(g.sum, 0, (size_t)(px * p.num_disp) * 4, ctx->stream) : hipSuccess;
    if (reset == hipSuccess && p.lr) reset = hipMemsetAsync(d.rmap, 0xFF, (size_t)px * 4, ctx->stream);      // KEY_NONE
    if (cost) stereo_census_launch(ctx, left, lstride, right, rstride, p.w, p.h);
    if (!sgm) {
        hipLaunchKernelGGL(STEREO_DENSE_KERNEL(np, false, cost), tiles, dim3(256), 0, ctx->stream, left, lstride, right, rstride, p,
                           d.rmap, d.best, d.status, (uint16_t *)nullptr);
        hipLaunchKernelGGL(k_stereo_dense_finish<uint2>, pixels, dim3(256), 0, ctx->stream, p, d.rmap, d.best, d.status, d.mm, d.disp);
    } else {
        const int dw = p.w - 2 * SR - p.min_disp, dh = p.h - 2 * SR;
        const int ndirs = __builtin_popcount((unsigned)sgm->mask), diagonal = sgm->mask & 0xF0, lines = diagonal ? dw + dh - 1 : dw > dh ? dw : dh;
        hipLaunchKernelGGL(STEREO_DENSE_KERNEL(np, true, cost), tiles, dim3(256), 0, ctx->stream, left, lstride, right, rstride, p,
                           (uint32_t *)nullptr, (uint2 *)nullptr, (uint8_t *)nullptr, g.vol);
        if (dw > 0)                                                   // else no pixel has a disparity to search: the domain is empty
            hipLaunchKernelGGL(STEREO_NP_KERNEL(np, k_sgm_paths), dim3(lines, ndirs), dim3(64), 0, ctx->stream, g.vol, g.sum, p, sgm->mask,
                               (unsigned)sgm->p1, (unsigned)sgm->p2);
        hipLaunchKernelGGL(STEREO_NP_KERNEL(np, k_sgm_select), tiles, dim3(256), 0, ctx->stream, g.sum, p, d.rmap, g.best, d.status);
        hipLaunchKernelGGL(k_stereo_dense_finish<uint4>, pixels, dim3(256), 0, ctx->stream, p, d.rmap, g.best, d.status, d.mm, d.disp);
    }
    const int filtered = speckle ? stereo_speckle_launch(ctx, p.w, p.h) : (int)RELOC_OK;
    reloc_prof_end(ctx, slot);
    HIP_TRY(reset);
    HIP_TRY(hipGetLastError());
    if (filtered) return filtered;
    d.w = p.w; d.h = p.h;
    if (sgm) { g.w = p.w; g.h = p.h; g.nd = p.num_disp; g.dmin = p.min_disp; }
    return RELOC_OK;
}

// the stateless image call: two gray planes of the caller's with one stride, explicit parameters, the three planes back
static int stereo_image(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, double fx, double baseline_m,
                        int min_disparity, int num_disparities, int uniqueness, int lr_check, int cost, const StereoSgm *sgm,
                        uint16_t *depth_mm, float *disparity, uint8_t *status)
{
    if (int rc = stereo_call_check(ctx, w, h, fx, baseline_m, min_disparity, num_disparities, uniqueness, lr_check, cost, sgm)) return rc;
    if (int rc = stereo_dense_alloc(ctx)) return rc;
    if (sgm)
        if (int rc = stereo_sgm_alloc(ctx, w, h, num_disparities)) return rc;
    const StereoState::Dense &d = ctx->stereo.dense;
    const int64_t bytes = (int64_t)(h - 1) * stride + w, px = (int64_t)w * h;
    HostStaging st{ctx};
    uint8_t *dl = st.slot<uint8_t>(0, bytes), *dr = st.slot<uint8_t>(1, bytes);
    if (st.rc) return st.finish();
    st.upload(dl, left, bytes);
    st.upload(dr, right, bytes);
    const StereoParams p = {fx, baseline_m, w, h, min_disparity, num_disparities, uniqueness, lr_check};
    st.run([&] { return stereo_dense_launch(ctx, dl, stride, dr, stride, p, cost, false, sgm); });
    st.download(depth_mm, d.mm, px * 2);
    if (disparity) st.download(disparity, d.disp, px * 4);
    if (status) st.download(status, d.status, px);
    return st.finish();
}

RELOC_API int reloc_stereo_depth_image(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, double fx,
                                       double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check,
                                       uint16_t *depth_mm, float *disparity, uint8_t *status)
{
    ARG_CHECK_CTX(ctx, left && right && depth_mm && w >= SP && h >= SP && stride >= w, "reloc_stereo_depth_image");
    return stereo_image(ctx, left, right, w, h, stride, fx, baseline_m, min_disparity, num_disparities, uniqueness, lr_check,
                        RELOC_STEREO_COST_SAD, nullptr, depth_mm, disparity, status);
}

RELOC_API int reloc_stereo_sgm_image(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, double fx,
                                     double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check,
                                     int path_mask, int p1, int p2, uint16_t *depth_mm, float *disparity, uint8_t *status)
{
    ARG_CHECK_CTX(ctx, left && right && depth_mm && w >= SP && h >= SP && stride >= w, "reloc_stereo_sgm_image");
    const StereoSgm sgm = {path_mask, p1, p2};
    return stereo_image(ctx, left, right, w, h, stride, fx, baseline_m, min_disparity, num_disparities, uniqueness, lr_check,
                        RELOC_STEREO_COST_SAD, &sgm, depth_mm, disparity, status);
}

RELOC_API int reloc_stereo_image_cost(reloc_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h, int stride, double fx,
                                      double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check, int cost,
                                      int path_mask, int p1, int p2, uint16_t *depth_mm, float *disparity, uint8_t *status)
{
    ARG_CHECK_CTX(ctx, left && right && depth_mm && w >= SP && h >= SP && stride >= w, "reloc_stereo_image_cost");
    const StereoSgm sgm = {path_mask, p1, p2};
    return stereo_image(ctx, left, right, w, h, stride, fx, baseline_m, min_disparity, num_disparities, uniqueness, lr_check, cost,
                        path_mask ? &sgm : nullptr, depth_mm, disparity, status);
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

int stereo_dense_frame(reloc_ctx *ctx, reloc_ctx *right, int w, int h, int order, int *ww, int *wh)
{
    StereoState &s = ctx->stereo;
    if (int rc = stereo_pair_check(ctx, right, w, h, ww, wh)) return rc;
    if (int rc = stereo_dense_alloc(ctx)) return rc;
    const uint8_t *plane[2];
    int pstride[2];
    if (int rc = stereo_gray_planes(ctx, right, ctx->frame_img, right->frame_img, w, h, *ww, *wh, order, plane, pstride)) return rc;
    const StereoParams p = {ctx->cam.K4[0], s.baseline, *ww, *wh, s.min_disp, s.num_disp, s.uniq, s.lr};
    const StereoSgm sgm = {s.sgm_paths == 4 ? 0x0F : 0xFF, s.sgm_p1, s.sgm_p2};
    return stereo_dense_launch(ctx, plane[0], pstride[0], plane[1], pstride[1], p, s.cost, s.speckle_window > 0, s.sgm_paths ? &sgm : nullptr);
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
    const StereoState::Dense *d = stereo_last_dense(ctx);
    if (!d) { reloc_set_error("no dense stereo pass on this context yet"); return RELOC_E_STATE; }
    const int64_t px = (int64_t)d->w * d->h;
    HostStaging st{ctx};
    if (depth_mm) st.download(depth_mm, d->mm, px * 2);
    if (disparity) st.download(disparity, d->disp, px * 4);
    if (status) st.download(status, d->status, px);
    if (int rc = st.finish()) return rc;
    if (w) *w = d->w;
    if (h) *h = d->h;
    return RELOC_OK;
}
