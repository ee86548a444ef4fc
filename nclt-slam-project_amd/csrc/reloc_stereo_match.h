// reloc_stereo_match.h -- the decision that the three stereo matchers make per pixel (include/reloc_spec.h, "STEREO", steps 2 to
// 8), stated once: k_stereo_depth of reloc_stereo.hip and k_stereo_dense, k_sgm_select and k_stereo_dense_finish of
// reloc_stereo_dense.hip differ in where the costs of a pixel come from, not in what follows from them.  Included by those
// two files only.
#pragma once
#include "reloc_teach.h"

constexpr int SR = RELOC_STEREO_R, SP = 2 * RELOC_STEREO_R + 1;     // radius and side of the patch
constexpr int STEREO_PASSES = RELOC_STEREO_NUM_DISP_MAX / 64;
constexpr unsigned KEY_NONE = 0xFFFFFFFFu;
static_assert(SP == 11 && SP * SP * 255 < (1 << 15) && RELOC_STEREO_MIN_DISPARITY_MAX + RELOC_STEREO_NUM_DISP_MAX < (1 << 11),
              "cost << 11 | disparity is a 26-bit key");
static_assert(STEREO_PASSES * 64 == RELOC_STEREO_NUM_DISP_MAX, "a lane holds num_disparities / 64 disparities");

struct StereoParams {
    double fx, baseline;
    int w, h;
    int min_disp, num_disp, uniq, lr;
};

// (cost, disparity) as one integer key: a minimum over keys is the lowest cost and, at a tie, the lowest disparity
__device__ __forceinline__ unsigned stereo_key(int cost, int d) { return ((unsigned)cost << 11) | (unsigned)d; }

// step 2: D = dmin .. dhi holds the three disparities that a parabola needs
__device__ __forceinline__ bool stereo_range_ok(int dmin, int dhi) { return dhi - dmin + 1 >= 3; }

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

// Steps 2, 4 and 5 of one pixel by its wave: cost[q] of lane l is the cost of d = dmin + 64 q + l, whatever it holds beyond
// dhi, the largest member of D (a register whose every d lies beyond dhi takes no part: NP may exceed the passes a pixel needs).
// The costs are the SADs C or the semi-global sums S, below 2^19 either way.  The result is the same in every lane: the status
// (OK, RANGE, EDGE or UNIQUENESS), d*, b = cost(d*) from step 4 on, a = cost(d* - 1) and c = cost(d* + 1) where the status is OK.
struct StereoPick { int status, dstar, a, b, c; };
template <int NP>
__device__ __forceinline__ StereoPick stereo_select(const int (&cost)[NP], int dmin, int dhi, int uniq, int lane)
{
    StereoPick s = {RELOC_STEREO_OK, 0, 0, 0, 0};
    if (!stereo_range_ok(dmin, dhi)) s.status = RELOC_STEREO_RANGE;
    else {
        unsigned key = KEY_NONE;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int d = dmin + 64 * q + lane;
            if (d <= dhi) key = min(key, stereo_key(cost[q], d));
        }
        key = wave_min_u32(key);
        s.dstar = (int)(key & 0x7FFu);
        s.b = (int)(key >> 11);
        if (s.dstar == dmin || s.dstar == dhi) s.status = RELOC_STEREO_EDGE;
        else {
            unsigned key2 = KEY_NONE;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const int d = dmin + 64 * q + lane;
                if (d <= dhi && abs(d - s.dstar) >= 2) key2 = min(key2, stereo_key(cost[q], d));
            }
            key2 = wave_min_u32(key2);
            if (key2 != KEY_NONE && (int)(key2 >> 11) * (100 - uniq) <= s.b * 100) s.status = RELOC_STEREO_UNIQUENESS;
            else {
                s.a = stereo_cost_of<NP>(cost, s.dstar - 1 - dmin);
                s.c = stereo_cost_of<NP>(cost, s.dstar + 1 - dmin);
            }
        }
    }
    return s;
}

// Steps 7 and 8: the parabola through a, b, c around d*, the disparity in float32, the depth in float64, millimetres.  status:
// OK, or FAR with mm and disp 0.
struct StereoDepth { int status; uint16_t mm; float disp; };
__device__ __forceinline__ StereoDepth stereo_depth_of(int dstar, int a, int b, int c, double fx, double baseline)
{
    const int den = a + c - 2 * b;
    const float delta = den <= 0 ? 0.f : __fdiv_rn((float)(a - c), (float)(2 * den));
    const float disp = __fadd_rn((float)dstar, delta);
    const double z = __ddiv_rn(__dmul_rn(fx, baseline), (double)disp);
    const double mm = rint(__dmul_rn(z, 1000.0));
    if (mm > 65535.0) return {RELOC_STEREO_FAR, 0, 0.f};
    return {RELOC_STEREO_OK, (uint16_t)mm, disp};
}
