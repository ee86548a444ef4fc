// reloc_census.hip -- the census transform on gfx950 (include/reloc_spec.h, "STEREO, census"): the data term of the three stereo
// matchers for pairs whose eyes are exposed unequally, and its parity tap (the cost setting itself is reloc_stereo.hip's).  The matchers
// themselves (reloc_stereo.hip, reloc_stereo_dense.hip) read a census plane as they read a gray plane; only their column cost
// differs (xor and popcount in v_sad_u8's place).
//   k_census   both eyes of a pass in one launch (blockIdx.y), each from a plane with its own stride into a dense plane of
//              stride w.  Memory-bound: a thread takes four consecutive bytes of the dense output (one dword store).  Where
//              the four lie in one row and their samples inside it, each of the three sampled rows (v - 2, v, v + 2, clamped
//              to the image) is two dword loads, u - 2 .. u + 5, and the eight comparisons per pixel run on bytes in
//              registers; the image's left and right edges, a dword that straddles two rows and the plane's last, partial
//              dword take the byte path with clamped coordinates.  No byte outside 0 <= x < w, 0 <= y < h is read.
#include "reloc_teach.h"

struct CensusEye { const uint8_t *src; int stride; uint8_t *dst; };

// T(I)[v, u] by the specification's letter: eight clamped byte loads around the centre
__device__ __forceinline__ uint32_t census_pixel(const uint8_t *__restrict__ img, int stride, int w, int h, int u, int v)
{
    const int um = max(u - 2, 0), up = min(u + 2, w - 1);
    const uint8_t *top = img + (size_t)max(v - 2, 0) * stride, *mid = img + (size_t)v * stride, *bot = img + (size_t)min(v + 2, h - 1) * stride;
    const uint32_t c = mid[u];
    return (uint32_t)(top[um] < c) | (uint32_t)(top[u] < c) << 1 | (uint32_t)(top[up] < c) << 2 | (uint32_t)(mid[um] < c) << 3 |
           (uint32_t)(mid[up] < c) << 4 | (uint32_t)(bot[um] < c) << 5 | (uint32_t)(bot[u] < c) << 6 | (uint32_t)(bot[up] < c) << 7;
}

// bytes x .. x + 7 of a row, any alignment
__device__ __forceinline__ uint64_t census_load8(const uint8_t *__restrict__ row, int x)
{
    uint64_t r;
    __builtin_memcpy(&r, row + x, 8);
    return r;
}

__global__ __launch_bounds__(256) void k_census(CensusEye e0, CensusEye e1, int w, int h)
{
    const CensusEye e = blockIdx.y ? e1 : e0;
    const int64_t n = (int64_t)w * h, i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const int v = (int)(i / w), u = (int)(i - (int64_t)v * w);
    if (u >= 2 && u + 5 < w) {               // the four pixels u .. u + 3 and their samples u - 2 .. u + 5 lie in row v
        const uint64_t top = census_load8(e.src + (size_t)max(v - 2, 0) * e.stride, u - 2);
        const uint64_t mid = census_load8(e.src + (size_t)v * e.stride, u - 2);
        const uint64_t bot = census_load8(e.src + (size_t)min(v + 2, h - 1) * e.stride, u - 2);
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t c = (uint32_t)(mid >> (8 * k + 16)) & 0xFFu;
            auto less = [&](uint64_t row, int b) { return (uint32_t)(((uint32_t)(row >> (8 * (k + b))) & 0xFFu) < c); };
            const uint32_t t = less(top, 0) | less(top, 2) << 1 | less(top, 4) << 2 | less(mid, 0) << 3 | less(mid, 4) << 4 | less(bot, 0) << 5 |
                               less(bot, 2) << 6 | less(bot, 4) << 7;
            out |= t << (8 * k);
        }
        *(uint32_t *)(e.dst + i) = out;       // dst is a block's buffer or a scratch slot: 256-byte aligned, i a multiple of 4
        return;
    }
    for (int k = 0; k < 4 && i + k < n; ++k) {
        int uk = u + k, vk = v;
        while (uk >= w) { uk -= w; ++vk; }   // w < 4: a dword spans more than two rows
        e.dst[i + k] = (uint8_t)census_pixel(e.src, e.stride, w, h, uk, vk);
    }
}

int stereo_census_alloc(reloc_ctx *ctx)
{
    StereoState::Census &c = ctx->stereo.census;
    if (c.block.p) return RELOC_OK;
    return c.block.layout(ctx, [&](BlockCarver &b) { stereo_census_lines(b, c, (int64_t)ctx->max_w * ctx->max_h); });
}

void stereo_census_launch(reloc_ctx *ctx, const uint8_t *&left, int &lstride, const uint8_t *&right, int &rstride, int w, int h)
{
    const StereoState::Census &c = ctx->stereo.census;
    const unsigned blocks = (unsigned)(((int64_t)w * h + 1023) / 1024);
    hipLaunchKernelGGL(k_census, dim3(blocks, 2), dim3(256), 0, ctx->stream, CensusEye{left, lstride, c.left}, CensusEye{right, rstride, c.right}, w, h);
    left = c.left; right = c.right;
    lstride = rstride = w;
}

RELOC_API int reloc_census(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride, uint8_t *out)
{
    ARG_CHECK_CTX(ctx, gray && out && w >= 1 && h >= 1 && stride >= w, "reloc_census");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    // the plane goes to the device as it lies at the caller's, padding included, and the kernel walks the caller's stride
    const int64_t bytes = (int64_t)(h - 1) * stride + w, px = (int64_t)w * h;
    HostStaging st{ctx};
    uint8_t *src = st.slot<uint8_t>(0, bytes), *dst = st.slot<uint8_t>(1, px);
    if (st.rc) return st.finish();
    st.upload(src, gray, bytes);
    const CensusEye e = {src, stride, dst};
    st.launch(k_census, dim3((unsigned)((px + 1023) / 1024), 1), dim3(256), e, e, w, h);
    st.download(out, dst, px);
    return st.finish();
}
