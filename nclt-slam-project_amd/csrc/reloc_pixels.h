// reloc_pixels.h -- the pixel helpers that the kernels of the image stages (reloc_image.hip) and of the ORB front end
// (reloc_orb.hip) share: the border rule, the fixed-point gray conversion and the pyramid's 4-pixel fetch.
#pragma once
#include "reloc_internal.h"

typedef uint32_t u32;

__device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) {
        if (p < 0) p = -p;
        if (p >= n) p = 2 * n - 2 - p;
    }
    return p;
}

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
