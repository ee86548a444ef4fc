// reloc_image.hip -- the image stages in front of ORB on gfx950, and the one place that orders them.
// A section per stage (kernels, host planning, one *_launch for n frames of equal geometry on one stream):
//   gray     cv2.cvtColor(.., COLOR_BGR2GRAY)   k_gray_plain; inside the chain the first kernel that reads the frame converts
//   BAYER    cv2.cvtColor(.., COLOR_Bayer??2BGR) k_bayer: a raw mosaic -> BGR (the shim) or -> gray (the stage)
//   PIXFMT   cv2.cvtColor(.., COLOR_BGRA2GRAY, COLOR_YUV2GRAY_YUY2, COLOR_YUV2BGR_YUY2 ..)   k_unpack: a packed frame -> gray
//            (the shim and the stage), k_yuv422_bgr: 4:2:2 -> BGR / RGB (the shim)
//   CLAHE    cv2.createCLAHE(..).apply          k_clahe_lut, k_clahe_apply
//   REMAP    cv2.remap, cv2.convertMaps         k_remap_u8, k_remap_nearest, k_convert_maps
//   RESIZE   cv2.resize                         k_resize_area, k_resize_linear, k_resize_nearest
// "image chain": [demosaic | unpack] -> resize -> rectify -> CLAHE on the frames in front of the pyramid (orb_run; 3-channel
// frames, raw mosaics with the Bayer stage on, or frames of the context's pixel format), resize -> rectify, both nearest, on
// the depth image of the recorder and the accumulation.  No other code states this order.
// "entry points": the host-pointer form of every stage (the cv2 shim) and the reloc_set_* / reloc_get_* of a context.
#include <float.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "reloc_internal.h"
#include "reloc_pixels.h"

// row stride of a stage's gray plane; bytes of one for the largest frame of a context (first enable of a stage)
static inline int plane_stride(int w) { return (w + 63) & ~63; }
static inline size_t stage_plane_bytes(const reloc_ctx *ctx) { return (size_t)plane_stride(ctx->max_w) * ctx->max_h; }

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

// the same on c's stream, device pointers: the right eye of a stereo pair whose chain has no stage on (reloc_stereo.hip)
int image_gray_plain(reloc_ctx *c, const uint8_t *src, int w, int h, int sstride, int order, uint8_t *dst)
{
    hipLaunchKernelGGL(k_gray_plain, dim3((w + 255) / 256, h), dim3(256), 0, c->stream, src, w, h, sstride, gray_flags(c, order), dst);
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

// ---- BAYER: cv2.cvtColor(raw, COLOR_Bayer??2BGR) (include/reloc_spec.h, "BAYER") ---------------------------------
// OpenCV's bilinear 8-bit demosaic, interior and border rule in one launch: output pixel (y, x) is the interior value at
// (clamp(y, 1, h - 2), clamp(x, 1, w - 2)) -- columns first, then rows, as the spec fills them.
//   k_bayer<OC, ALIGNED>   4 output pixels per lane along x from three source rows.  ALIGNED (w % 4 == 0, rows on dwords):
//                          per row the lane's dword and its two neighbours (one halo byte each); the border columns are then
//                          pixels 0 and 3 of the first / last quad and take their neighbour's triple.  Otherwise (odd widths,
//                          strided or odd sources): the nine bytes around every clamped pixel through the cache.
//                          OC = 3: interleaved BGR (the shim).  OC = 1: gray_fixed of the triple with the coefficient flags --
//                          the stage at the head of the image chain, byte for byte cvtColor(cvtColor(raw, Bayer2BGR), BGR2GRAY).
// The pattern is two launch-uniform parity bits, not four instantiations: green_par = parity of x + y at the green sites,
// blue_par = parity of the rows that hold blue sites; every site kind is computed by the same selects.  Frame-batched
// (blockIdx.y = frame); a single frame is a batch of one.
struct BayerFrames { const uint8_t *src[RELOC_BATCH_MAX]; uint8_t *dst[RELOC_BATCH_MAX]; };

// the triple of one site from its 3 x 3 neighbourhood t (top), m (middle), b (bottom), columns 0..2
__device__ __forceinline__ void bayer_site(const int (&t)[3], const int (&m)[3], const int (&b)[3], bool green, bool blue_row,
                                           int &vb, int &vg, int &vr)
{
    const int c = m[1];
    const int hor = (m[0] + m[2] + 1) >> 1, ver = (t[1] + b[1] + 1) >> 1;
    const int cross = (t[1] + b[1] + m[0] + m[2] + 2) >> 2, diag = (t[0] + t[2] + b[0] + b[2] + 2) >> 2;
    const int row_col = green ? hor : c;          // the colour of this row's red / blue sites
    const int other = green ? ver : diag;         // the colour of the neighbouring rows' red / blue sites
    vg = green ? c : cross;
    vb = blue_row ? row_col : other;
    vr = blue_row ? other : row_col;
}

template <int OC, bool ALIGNED>
__global__ __launch_bounds__(256) void k_bayer(BayerFrames F, int w, int h, int sstride, int dstride, int green_par, int blue_par,
                                               int flags)
{
    const int quads = (w + 3) >> 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= quads * h) return;
    const int y = q / quads, x4 = 4 * (q - y * quads);
    const int yc = min(max(y, 1), h - 2);
    const bool blue_row = ((yc ^ blue_par) & 1) == 0;
    const uint8_t *src = F.src[blockIdx.y];
    int vb[4], vg[4], vr[4];
    if (ALIGNED) {
        // columns x4 - 1 .. x4 + 4 of rows yc - 1 .. yc + 1; a halo byte outside the image is 0 and feeds a border pixel only
        int v[3][6];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const u32 *row = reinterpret_cast<const u32 *>(src + (size_t)(yc - 1 + r) * sstride + x4);
            const u32 prev = x4 > 0 ? row[-1] : 0u, cur = row[0], next = x4 + 4 < w ? row[1] : 0u;
            v[r][0] = prev >> 24;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[r][1 + k] = (cur >> (8 * k)) & 255u;
            v[r][5] = next & 255u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t[3] = {v[0][k], v[0][k + 1], v[0][k + 2]}, m[3] = {v[1][k], v[1][k + 1], v[1][k + 2]};
            const int b[3] = {v[2][k], v[2][k + 1], v[2][k + 2]};
            bayer_site(t, m, b, (((x4 + k) ^ yc ^ green_par) & 1) == 0, blue_row, vb[k], vg[k], vr[k]);
        }
        if (x4 == 0) { vb[0] = vb[1]; vg[0] = vg[1]; vr[0] = vr[1]; }              // column 0 copies column 1
        if (x4 + 4 == w) { vb[3] = vb[2]; vg[3] = vg[2]; vr[3] = vr[2]; }          // column w - 1 copies column w - 2
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xc = min(max(x4 + k, 1), w - 2);          // also keeps the reads of a pixel beyond w inside the row
            const uint8_t *p = src + (size_t)(yc - 1) * sstride + (xc - 1);
            const int t[3] = {p[0], p[1], p[2]}, m[3] = {p[sstride], p[sstride + 1], p[sstride + 2]};
            const int b[3] = {p[2 * (size_t)sstride], p[2 * (size_t)sstride + 1], p[2 * (size_t)sstride + 2]};
            bayer_site(t, m, b, ((xc ^ yc ^ green_par) & 1) == 0, blue_row, vb[k], vg[k], vr[k]);
        }
    }
    uint8_t *dst = F.dst[blockIdx.y] + (size_t)y * dstride + OC * x4;
    if (OC == 1) {
        u32 out = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x4 + k < w) out |= (u32)gray_fixed(vb[k], vg[k], vr[k], flags) << (8 * k);
        if ((dstride & 3) == 0) {
            *reinterpret_cast<u32 *>(dst) = out;       // the row holds round4(w) bytes: dstride >= w and a multiple of 4
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x4 + k < w) dst[k] = (uint8_t)(out >> (8 * k));
        }
    } else if (ALIGNED && (dstride & 3) == 0) {
        u32 *d4 = reinterpret_cast<u32 *>(dst);        // 12 bytes of 4 whole pixels (w % 4 == 0)
        d4[0] = (u32)vb[0] | (u32)vg[0] << 8 | (u32)vr[0] << 16 | (u32)vb[1] << 24;
        d4[1] = (u32)vg[1] | (u32)vr[1] << 8 | (u32)vb[2] << 16 | (u32)vg[2] << 24;
        d4[2] = (u32)vr[2] | (u32)vb[3] << 8 | (u32)vg[3] << 16 | (u32)vr[3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x4 + k < w) { dst[3 * k] = (uint8_t)vb[k]; dst[3 * k + 1] = (uint8_t)vg[k]; dst[3 * k + 2] = (uint8_t)vr[k]; }
    }
}

static inline bool bayer_code_ok(int code) { return code >= RELOC_BAYER_BG2BGR && code <= RELOC_BAYER_GR2BGR; }

// one demosaic launch for n mosaics of w x h (>= 3 x 3) on stream st; oc: 3 -> interleaved BGR, 1 -> gray (flags: the
// coefficient set; the channel-order bit has no meaning for a mosaic)
static int bayer_launch(hipStream_t st, const BayerFrames &F, int n, int w, int h, int sstride, int dstride, int code, int oc, int flags)
{
    bool aligned = w % 4 == 0 && sstride % 4 == 0;
    for (int f = 0; f < n; ++f) aligned = aligned && ((uintptr_t)F.src[f]) % 4 == 0 && ((uintptr_t)F.dst[f]) % 4 == 0;
    // BG (46): R G / G B   GB (47): G R / B G   RG (48): B G / G R   GR (49): G B / R G
    const int green_par = (code & 1) ^ 1, blue_par = ((code - RELOC_BAYER_BG2BGR) >> 1) ^ 1;
    auto kern = oc == 3 ? (aligned ? k_bayer<3, true> : k_bayer<3, false>) : (aligned ? k_bayer<1, true> : k_bayer<1, false>);
    hipLaunchKernelGGL(kern, dim3((((w + 3) / 4) * h + 255) / 256, n), dim3(256), 0, st, F, w, h, sstride, dstride, green_par, blue_par,
                       flags & RELOC_GRAY_FLAG_15BIT);
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

// ---- PIXFMT: packed camera frames (include/reloc_spec.h, "PIXEL FORMATS") ---------------------------------------------
//   k_unpack<FMT, ALIGNED>   the gray plane of a packed frame, 4 output pixels per lane, one dword store.  YUYV / UYVY: the Y
//                            bytes (cvtColor(.., COLOR_YUV2GRAY_YUY2 / _UYVY)), 8 source bytes per lane.  BGRA / RGBA:
//                            gray_fixed of the first three channels with the coefficient flag, alpha ignored
//                            (COLOR_BGRA2GRAY / COLOR_RGBA2GRAY), 16 source bytes per lane.  ALIGNED (w % 4 == 0, rows on 8 /
//                            16 bytes): one 64-bit / 128-bit load per lane, consecutive lanes consecutive addresses.
//                            Otherwise the bytes of the pixels inside the row, through the cache (the guards of
//                            pyr_fetch<CH, false>).  It is the stage at the head of the image chain, in the Bayer stage's place, and
//                            reloc_cvt_gray_u8.  Grid (x, frame, row): no division; a single frame is a batch of one.
//   k_yuv422_bgr             cvtColor(.., COLOR_YUV2BGR_YUY2 / _UYVY and the 2RGB twins): one pixel pair per lane, 4 bytes in,
//                            6 out, OpenCV's fixed-point BT.601.  Serves reloc_yuv422_bgr_u8 only.
// No LDS, no scratch.  mono8 frames need no kernel: they are gray planes.
struct UnpackFrames { const uint8_t *src[RELOC_BATCH_MAX]; uint8_t *dst[RELOC_BATCH_MAX]; };
constexpr int UNPACK_BS = 64;          // one wave = 256 pixels of a row: 640 and 1280 columns waste 17 % and 0 % of their lanes

template <int FMT, bool ALIGNED>
__global__ __launch_bounds__(UNPACK_BS) void k_unpack(UnpackFrames F, int w, int sstride, int dstride, int flags)
{
    constexpr int BPP = (FMT == RELOC_FMT_YUYV || FMT == RELOC_FMT_UYVY) ? 2 : 4;
    const int x4 = 4 * (blockIdx.x * UNPACK_BS + threadIdx.x), y = blockIdx.z;
    if (x4 >= w) return;
    const uint8_t *sp = F.src[blockIdx.y] + (size_t)y * sstride + (size_t)BPP * x4;
    u32 d[BPP];         // the 4 pixels' bytes; a pixel beyond w reads as 0
    if (ALIGNED) {
        if constexpr (BPP == 2) { const uint2 v = *reinterpret_cast<const uint2 *>(sp); d[0] = v.x; d[1] = v.y; }
        else { const uint4 v = *reinterpret_cast<const uint4 *>(sp); d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
    } else {
#pragma unroll
        for (int i = 0; i < BPP; ++i) d[i] = 0;
#pragma unroll
        for (int k = 0; k < 4 * BPP; ++k)
            if (x4 + k / BPP < w) d[k >> 2] |= (u32)sp[k] << (8 * (k & 3));
    }
    u32 out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if constexpr (BPP == 2) {
            const int bi = 2 * k + (FMT == RELOC_FMT_UYVY ? 1 : 0);
            out |= ((d[bi >> 2] >> (8 * (bi & 3))) & 255u) << (8 * k);
        } else {
            const int c0 = d[k] & 255u, c1 = (d[k] >> 8) & 255u, c2 = (d[k] >> 16) & 255u;
            const int g = FMT == RELOC_FMT_RGBA ? gray_fixed(c2, c1, c0, flags) : gray_fixed(c0, c1, c2, flags);
            if (x4 + k < w) out |= (u32)g << (8 * k);
        }
    }
    uint8_t *dst = F.dst[blockIdx.y] + (size_t)y * dstride + x4;
    if ((dstride & 3) == 0) {
        *reinterpret_cast<u32 *>(dst) = out;       // the row holds round4(w) bytes: dstride >= w and a multiple of 4
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x4 + k < w) dst[k] = (uint8_t)(out >> (8 * k));
    }
}

__device__ __forceinline__ int yuv_sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// src: dense rows of 2 w bytes on a dword (w is even), dst: dense rows of 3 w bytes on a word -- the staging plane and a
// scratch slot of reloc_yuv422_bgr_u8.  uyvy: the Y bytes are the odd ones; rgb: R first
__global__ __launch_bounds__(256) void k_yuv422_bgr(const uint8_t *__restrict__ src, int w, int uyvy, int rgb, uint8_t *__restrict__ dst)
{
    const int p = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (2 * p >= w) return;
    const u32 q = reinterpret_cast<const u32 *>(src + (size_t)y * 2 * w)[p];
    const int b0 = q & 255u, b1 = (q >> 8) & 255u, b2 = (q >> 16) & 255u, b3 = q >> 24;
    const int u = (uyvy ? b0 : b1) - 128, v = (uyvy ? b2 : b3) - 128;
    const int ruv = (1 << (RELOC_YUV_SHIFT - 1)) + RELOC_YUV_CVR * v;
    const int guv = (1 << (RELOC_YUV_SHIFT - 1)) + RELOC_YUV_CVG * v + RELOC_YUV_CUG * u;
    const int buv = (1 << (RELOC_YUV_SHIFT - 1)) + RELOC_YUV_CUB * u;
    int c[6];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int yy = max(0, (k ? (uyvy ? b3 : b2) : (uyvy ? b1 : b0)) - 16) * RELOC_YUV_CY;
        const int B = yuv_sat8((yy + buv) >> RELOC_YUV_SHIFT), G = yuv_sat8((yy + guv) >> RELOC_YUV_SHIFT);
        const int R = yuv_sat8((yy + ruv) >> RELOC_YUV_SHIFT);
        c[3 * k] = rgb ? R : B; c[3 * k + 1] = G; c[3 * k + 2] = rgb ? B : R;
    }
    uint16_t *d = reinterpret_cast<uint16_t *>(dst + (size_t)y * 3 * w) + 3 * p;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = (uint16_t)(c[2 * k] | c[2 * k + 1] << 8);
}

static inline bool pixfmt_packed(int fmt) { return fmt >= RELOC_FMT_BGRA && fmt <= RELOC_FMT_UYVY; }
static inline bool pixfmt_422(int fmt) { return fmt == RELOC_FMT_YUYV || fmt == RELOC_FMT_UYVY; }

// one unpack launch for n packed frames of w x h on stream st (w even for 4:2:2: the callers check); flags: the coefficient set
static int unpack_launch(hipStream_t st, const UnpackFrames &F, int n, int w, int h, int sstride, int dstride, int fmt, int flags)
{
    const int vec = pixfmt_422(fmt) ? 8 : 16;           // bytes of 4 pixels
    bool aligned = w % 4 == 0 && sstride % vec == 0;
    for (int f = 0; f < n; ++f) aligned = aligned && ((uintptr_t)F.src[f]) % vec == 0 && ((uintptr_t)F.dst[f]) % 4 == 0;
#define UNPACK_KERN(FMT) (aligned ? k_unpack<FMT, true> : k_unpack<FMT, false>)
    auto kern = fmt == RELOC_FMT_BGRA ? UNPACK_KERN(RELOC_FMT_BGRA) : fmt == RELOC_FMT_RGBA ? UNPACK_KERN(RELOC_FMT_RGBA)
                : fmt == RELOC_FMT_YUYV ? UNPACK_KERN(RELOC_FMT_YUYV) : UNPACK_KERN(RELOC_FMT_UYVY);
#undef UNPACK_KERN
    hipLaunchKernelGGL(kern, dim3(((w + 3) / 4 + UNPACK_BS - 1) / UNPACK_BS, n, h), dim3(UNPACK_BS), 0, st, F, w, sstride, dstride,
                       flags & RELOC_GRAY_FLAG_15BIT);
    HIP_TRY(hipGetLastError());
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

// one nearest remap of a single frame on stream st; elem: bytes per channel value (2 = the 16-bit depth image)
static int remap_nearest_launch(hipStream_t st, const RemapFrames &F, const RemapGeom &g, int channels, int elem)
{
    auto kern = elem == 2 ? k_remap_nearest<uint16_t, 1> : channels == 1 ? k_remap_nearest<uint8_t, 1> : k_remap_nearest<uint8_t, 3>;
    hipLaunchKernelGGL(kern, dim3((g.dw + 255) / 256, 1, g.dh), dim3(256), 0, st, F, g);
    HIP_TRY(hipGetLastError());
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

// ---- image chain ----------------------------------------------------------------------------------------------
// bytes per pixel of the frames that enter the chain through orb_run: a raw mosaic with the Bayer stage on, else those of
// the context's pixel format (3 channels by default)
int image_chain_frame_bpp(const reloc_ctx *c) { return c->img.bayer.on() ? 1 : c->img.pixfmt.bpp(); }

// a frame or depth image of *w x *h enters the downscale stage r: *w x *h becomes the working frame
static int resize_enter(const ResizeStage &r, int *w, int *h)
{
    if (*w == r.sw && *h == r.sh) { *w = r.dw; *h = r.dh; return RELOC_OK; }
    reloc_set_error("frame %dx%d differs from the source size %dx%d of the downscale stage (reloc_set_resize)", *w, *h, r.sw, r.sh);
    return RELOC_E_ARG;
}
// ... and the rectification r
static int rectify_enter(const RectifyStage &r, int w, int h)
{
    if (w == r.w && h == r.h) return RELOC_OK;
    reloc_set_error("frame %dx%d differs from the rectification map %dx%d (reloc_set_rectify_map)", w, h, r.w, r.h);
    return RELOC_E_ARG;
}

static int batch_unequal(const char *what) { reloc_set_error("orb batch: contexts %s", what); return RELOC_E_STATE; }

// Before orb_prepare: the contexts agree on the Bayer stage, the pixel format and the downscale stage, a frame of the chain
// has the latter's source size (and an even width in a 4:2:2 format); w x h becomes the working frame, which orb_prepare and
// everything downstream see.
int image_chain_check(reloc_ctx *const *ctxs, int n, bool chain, int *w, int *h)
{
    const auto &s0 = ctxs[0]->img;
    for (int f = 0; f < n; ++f) {
        if (!ctxs[f]->img.resize.same(s0.resize)) return batch_unequal("with and without the downscale stage, or with unequal sizes (reloc_set_resize)");
        if (!ctxs[f]->img.bayer.same(s0.bayer)) return batch_unequal("with and without the Bayer stage, or of unequal patterns (reloc_set_bayer)");
        if (!ctxs[f]->img.pixfmt.same(s0.pixfmt)) return batch_unequal("of unequal pixel formats (reloc_set_pixel_format)");
    }
    if (!chain) return RELOC_OK;
    if (s0.pixfmt.yuv422() && (*w & 1)) { reloc_set_error("bad argument: a 4:2:2 frame (reloc_set_pixel_format) has an even width, not %d", *w); return RELOC_E_ARG; }
    if (!s0.resize.on()) return RELOC_OK;
    if (int rc = resize_enter(s0.resize, w, h)) return rc;
    if (*w < 64 || *h < 64) { reloc_set_error("bad argument: the working frame %dx%d of the downscale stage is below 64x64", *w, *h); return RELOC_E_ARG; }
    return RELOC_OK;
}

// Behind orb_prepare of context f, where these checks have always stood (a call's errors keep their order): f agrees with
// context 0 on rectification and CLAHE; behind the last context, the working frame of the chain has the size of the map.
int image_chain_check_prepared(reloc_ctx *const *ctxs, int f, int n, bool chain, int w, int h)
{
    const auto &s0 = ctxs[0]->img, &s = ctxs[f]->img;
    if (!s.rectify.same(s0.rectify)) return batch_unequal("with and without a rectification map, or with maps of unequal size (reloc_set_rectify_map)");
    if (!s.clahe.same(s0.clahe)) return batch_unequal("of unequal CLAHE settings (reloc_set_clahe)");
    return f == n - 1 && chain && s0.rectify.on() ? rectify_enter(s0.rectify, w, h) : RELOC_OK;
}

// The gray half, on the stream of the (checked) contexts: frames *srcs of sw x sh, rows of *stride bytes (chain: 3 channels,
// raw mosaics with the Bayer stage on, or the contexts' pixel format), go through the stages that are on, each into its
// context's plane; the first one converts to gray (a mono8 frame is gray).  Afterwards *srcs (= planes, the caller's array) /
// *stride / *channels describe the last plane written, or the frame itself where no stage ran.  A caller's gray plane
// (!chain) passes untouched.
int image_chain_gray(reloc_ctx *const *ctxs, int n, bool chain, const uint8_t *const **srcs, int sw, int sh, int w, int h,
                     int *stride, int *channels, int flags, const uint8_t **planes)
{
    *channels = 1;
    if (!chain) return RELOC_OK;
    const reloc_ctx *c0 = ctxs[0];
    const auto &s0 = c0->img;
    if (s0.pixfmt.fmt != RELOC_FMT_MONO8) *channels = 3;       // a packed frame or a mosaic: its head stage never reads this
    enum { STAGE_BAYER, STAGE_UNPACK, STAGE_RESIZE, STAGE_RECTIFY, STAGE_CLAHE, N_STAGES };       // the order of the chain
    const bool on[N_STAGES] = {s0.bayer.on(), s0.pixfmt.on(), s0.resize.on(), s0.rectify.on(), s0.clahe.on()};
    for (int s = 0; s < N_STAGES; ++s) {
        if (!on[s]) continue;
        const uint8_t *const *in = *srcs;
        const int cs = plane_stride(s <= STAGE_UNPACK ? sw : w);       // the plane of a head stage has the source size
        int rc;
        if (s == STAGE_BAYER) {
            BayerFrames F = {};
            for (int f = 0; f < n; ++f) { F.src[f] = in[f]; planes[f] = F.dst[f] = ctxs[f]->img.bayer.plane; }
            rc = bayer_launch(c0->stream, F, n, sw, sh, *stride, cs, s0.bayer.code, 1, flags);
        } else if (s == STAGE_UNPACK) {
            UnpackFrames F = {};
            for (int f = 0; f < n; ++f) { F.src[f] = in[f]; planes[f] = F.dst[f] = ctxs[f]->img.pixfmt.plane; }
            rc = unpack_launch(c0->stream, F, n, sw, sh, *stride, cs, s0.pixfmt.fmt, flags);
        } else if (s == STAGE_RESIZE) {
            ResizeFrames F = {};
            for (int f = 0; f < n; ++f) { F.src[f] = in[f]; F.tab[f] = ctxs[f]->img.resize.tab; planes[f] = F.dst[f] = ctxs[f]->img.resize.plane; }
            ResizePlan P;
            P.kind = s0.resize.kind; P.isx = s0.resize.isx; P.isy = s0.resize.isy;
            rc = resize_launch(c0->stream, F, n, P, sw, sh, *stride, w, h, cs, *channels, 1, *channels == 3, flags);
        } else if (s == STAGE_RECTIFY) {
            RemapFrames F = {};
            for (int f = 0; f < n; ++f) {
                const RectifyStage &r = ctxs[f]->img.rectify;
                F.src[f] = in[f]; F.xy[f] = r.xy; F.alpha[f] = r.alpha; planes[f] = F.dst[f] = r.plane;
            }
            rc = remap_launch(c0->stream, F, n, RemapGeom{w, h, *stride, w, h, cs, 0}, *channels, *channels == 3, flags);
        } else {
            ClaheFrames F = {};
            for (int f = 0; f < n; ++f) { F.src[f] = in[f]; F.lut[f] = ctxs[f]->img.clahe.lut; planes[f] = F.dst[f] = ctxs[f]->img.clahe.plane; }
            rc = clahe_launch(c0->stream, F, n, clahe_geom(w, h, s0.clahe.clip, s0.clahe.tx, s0.clahe.ty), *channels, *stride, flags, cs);
        }
        if (rc) return rc;
        *srcs = planes; *stride = cs; *channels = 1;
    }
    return RELOC_OK;
}

// The depth half (reloc_record_frame, reloc_tick_accumulate_dev): a depth image (uint16 mm, dense rows) follows the frame,
// nearest both times, border 0 = "no depth"; *w x *h becomes the working frame, *out the last plane written (or depth_dev).
int image_chain_depth(reloc_ctx *ctx, const uint16_t *depth_dev, int *w, int *h, const uint16_t **out)
{
    *out = depth_dev;
    if (const ResizeStage &r = ctx->img.resize; r.on()) {
        const int sw = *w, sh = *h;
        if (int rc = resize_enter(r, w, h)) return rc;
        ResizeFrames F = {};
        F.src[0] = (const uint8_t *)*out; F.tab[0] = r.ntab; F.dst[0] = (uint8_t *)r.depth;
        ResizePlan P;
        P.kind = RESIZE_NEAREST;
        if (int rc = resize_launch(ctx->stream, F, 1, P, sw, sh, sw, *w, *h, *w, 1, 2, false, 0)) return rc;
        *out = r.depth;
    }
    if (const RectifyStage &r = ctx->img.rectify; r.on()) {
        if (int rc = rectify_enter(r, *w, *h)) return rc;
        RemapFrames F = {};
        F.src[0] = (const uint8_t *)*out; F.xy[0] = r.xy; F.dst[0] = (uint8_t *)r.depth;
        if (int rc = remap_nearest_launch(ctx->stream, F, RemapGeom{*w, *h, *w, *w, *h, *w, 0}, 1, 2)) return rc;      // strides in elements
        *out = r.depth;
    }
    return RELOC_OK;
}

// ---- entry points ---------------------------------------------------------------------------------------------
// A host-pointer entry point stages through HostStaging: the source into ctx->frame_img with dense rows, tables and the
// destination in scratch slots.  Capacity checks and slot numbers stay with the entry point.
RELOC_API int reloc_gray_u8(reloc_ctx *ctx, const uint8_t *img, int w, int h, int stride, int order, uint8_t *gray)
{
    ARG_CHECK_CTX(ctx, img && gray && w > 0 && h > 0 && stride >= 3 * w, "reloc_gray_u8");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    HostStaging st{ctx};
    uint8_t *dout = st.slot<uint8_t>(0, (int64_t)w * h);
    st.upload_rows(ctx->frame_img, img, w * 3, h, stride);
    st.launch(k_gray_plain, dim3((w + 255) / 256, h), dim3(256), ctx->frame_img, w, h, w * 3, gray_flags(ctx, order), dout);
    st.download(gray, dout, (int64_t)w * h);
    return st.finish();
}

// ---- Bayer entry points --------------------------------------------------------------------------------
RELOC_API int reloc_bayer_u8(reloc_ctx *ctx, const uint8_t *raw, int w, int h, int stride, int code, uint8_t *out_bgr)
{
    ARG_CHECK_CTX(ctx, raw && out_bgr && w >= 3 && h >= 3 && stride >= w, "reloc_bayer_u8: NULL pointer, or a mosaic below 3 x 3");
    ARG_CHECK(bayer_code_ok(code), "reloc_bayer_u8: code must be one of COLOR_BayerBG2BGR .. COLOR_BayerGR2BGR (46..49)");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    HostStaging st{ctx};
    uint8_t *dout = st.slot<uint8_t>(0, (int64_t)w * h * 3);
    st.upload_rows(ctx->frame_img, raw, w, h, stride);
    BayerFrames F = {};
    F.src[0] = ctx->frame_img; F.dst[0] = dout;
    st.run([&] { return bayer_launch(ctx->stream, F, 1, w, h, w, 3 * w, code, 3, 0); });
    st.download(out_bgr, dout, (int64_t)w * h * 3);
    return st.finish();
}

RELOC_API int reloc_set_bayer(reloc_ctx *ctx, int code)
{
    ARG_CHECK_CTX(ctx, true, "ctx is NULL");
    ARG_CHECK(code == 0 || bayer_code_ok(code), "reloc_set_bayer: code must be 0 (off) or one of COLOR_BayerBG2BGR .. COLOR_BayerGR2BGR (46..49)");
    BayerStage &b = ctx->img.bayer;
    if (code && ctx->img.pixfmt.fmt != RELOC_FMT_BGR) {
        reloc_set_error("reloc_set_bayer: a pixel format is set (reloc_set_pixel_format); a frame is a mosaic or of a pixel format, not both");
        return RELOC_E_STATE;
    }
    if (code && !b.plane)       // first enable: the gray plane of the largest mosaic
        if (int rc = b.block.layout(ctx, [&](BlockCarver &c) { c.own(b.plane, stage_plane_bytes(ctx)); })) return rc;
    b.code = code;
    return RELOC_OK;
}

RELOC_API int reloc_get_bayer(reloc_ctx *ctx, int32_t *code)
{
    ARG_CHECK_CTX(ctx, code, "reloc_get_bayer");
    *code = ctx->img.bayer.code;
    return RELOC_OK;
}

// ---- pixel format entry points ------------------------------------------------------------------------------
// the staging plane holds frames of bpp bytes per pixel: 3 from creation, grown once, to 4; nothing of it survives the growth
int frame_img_reserve(reloc_ctx *ctx, int bpp)
{
    if (bpp <= ctx->frame_img_bpp) return RELOC_OK;
    if (int rc = ctx->frame_block.layout(ctx, [&](BlockCarver &c) { c.own(ctx->frame_img, (int64_t)ctx->max_w * ctx->max_h * bpp); })) return rc;
    ctx->frame_img_bpp = bpp;
    return RELOC_OK;
}

RELOC_API int reloc_cvt_gray_u8(reloc_ctx *ctx, const uint8_t *src, int w, int h, int stride, int fmt, uint8_t *out)
{
    ARG_CHECK_CTX(ctx, src && out && w >= 1 && h >= 1, "reloc_cvt_gray_u8");
    ARG_CHECK(pixfmt_packed(fmt), "reloc_cvt_gray_u8: fmt must be RELOC_FMT_BGRA, RELOC_FMT_RGBA, RELOC_FMT_YUYV or RELOC_FMT_UYVY");
    const int bpp = pixfmt_422(fmt) ? 2 : 4;
    ARG_CHECK(!(pixfmt_422(fmt) && (w & 1)), "reloc_cvt_gray_u8: a 4:2:2 frame has an even width");
    ARG_CHECK(stride >= w * bpp, "reloc_cvt_gray_u8: the stride is below the row");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    if (int rc = frame_img_reserve(ctx, bpp)) return rc;
    HostStaging st{ctx};
    uint8_t *dout = st.slot<uint8_t>(0, (int64_t)w * h);
    st.upload_rows(ctx->frame_img, src, w * bpp, h, stride);
    UnpackFrames F = {};
    F.src[0] = ctx->frame_img; F.dst[0] = dout;
    st.run([&] { return unpack_launch(ctx->stream, F, 1, w, h, w * bpp, w, fmt, gray_flags(ctx, 0)); });
    st.download(out, dout, (int64_t)w * h);
    return st.finish();
}

RELOC_API int reloc_yuv422_bgr_u8(reloc_ctx *ctx, const uint8_t *src, int w, int h, int stride, int fmt, int order, uint8_t *out)
{
    ARG_CHECK_CTX(ctx, src && out && w >= 1 && h >= 1, "reloc_yuv422_bgr_u8");
    ARG_CHECK(pixfmt_422(fmt), "reloc_yuv422_bgr_u8: fmt must be RELOC_FMT_YUYV or RELOC_FMT_UYVY");
    ARG_CHECK(!(w & 1), "reloc_yuv422_bgr_u8: a 4:2:2 frame has an even width");
    ARG_CHECK(stride >= w * 2, "reloc_yuv422_bgr_u8: the stride is below the row");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    HostStaging st{ctx};
    uint8_t *dout = st.slot<uint8_t>(0, (int64_t)w * h * 3);
    st.upload_rows(ctx->frame_img, src, w * 2, h, stride);
    st.launch(k_yuv422_bgr, dim3((w / 2 + 255) / 256, h), dim3(256), ctx->frame_img, w, fmt == RELOC_FMT_UYVY, order & 1, dout);
    st.download(out, dout, (int64_t)w * h * 3);
    return st.finish();
}

RELOC_API int reloc_set_pixel_format(reloc_ctx *ctx, int fmt)
{
    ARG_CHECK_CTX(ctx, true, "ctx is NULL");
    ARG_CHECK(fmt >= RELOC_FMT_BGR && fmt <= RELOC_FMT_UYVY, "reloc_set_pixel_format: fmt must be one of RELOC_FMT_BGR (0, the default) .. RELOC_FMT_UYVY");
    PixfmtStage &p = ctx->img.pixfmt;
    if (fmt && ctx->img.bayer.on()) {
        reloc_set_error("reloc_set_pixel_format: the Bayer stage is on (reloc_set_bayer); a frame is a mosaic or of a pixel format, not both");
        return RELOC_E_STATE;
    }
    if (pixfmt_packed(fmt)) {
        if (!p.plane)           // first enable of a packed format: the gray plane of the largest frame
            if (int rc = p.block.layout(ctx, [&](BlockCarver &c) { c.own(p.plane, stage_plane_bytes(ctx)); })) return rc;
        if (int rc = frame_img_reserve(ctx, pixfmt_422(fmt) ? 2 : 4)) return rc;
    }
    p.fmt = fmt;
    return RELOC_OK;
}

RELOC_API int reloc_get_pixel_format(reloc_ctx *ctx, int32_t *fmt)
{
    ARG_CHECK_CTX(ctx, fmt, "reloc_get_pixel_format");
    *fmt = ctx->img.pixfmt.fmt;
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
    ClaheStage &c = ctx->img.clahe;
    if (tiles_x == 0 && tiles_y == 0) {
        c.clip = 0.0; c.tx = c.ty = 0;
        return RELOC_OK;
    }
    ARG_CHECK(clahe_args_ok(clip_limit, tiles_x, tiles_y),
              "reloc_set_clahe: tiles_x and tiles_y must both be 0 (off) or both in 1..64, and clip_limit finite");
    if (!c.plane)       // first enable, one block: the plane of the largest frame, then the LUTs of the largest grid
        if (int rc = c.block.layout(ctx, [&](BlockCarver &b) {
                b.own(c.plane, stage_plane_bytes(ctx));
                b.aligned<64>(c.lut, (int64_t)CLAHE_MAX_TILES * CLAHE_MAX_TILES * 256);
            })) return rc;
    c.clip = clip_limit == 0.0 ? 0.0 : clip_limit;     // -0 -> +0: equal settings compare equal
    c.tx = tiles_x; c.ty = tiles_y;
    return RELOC_OK;
}

RELOC_API int reloc_get_clahe(reloc_ctx *ctx, double *clip_limit, int32_t *tiles_x, int32_t *tiles_y)
{
    ARG_CHECK_CTX(ctx, clip_limit && tiles_x && tiles_y, "reloc_get_clahe");
    *clip_limit = ctx->img.clahe.clip; *tiles_x = ctx->img.clahe.tx; *tiles_y = ctx->img.clahe.ty;
    return RELOC_OK;
}

RELOC_API int reloc_clahe_u8(reloc_ctx *ctx, const uint8_t *gray, int w, int h, int stride, double clip_limit, int tiles_x,
                             int tiles_y, uint8_t *out)
{
    ARG_CHECK_CTX(ctx, gray && out && w >= 1 && h >= 1 && stride >= w, "reloc_clahe_u8");
    ARG_CHECK(clahe_args_ok(clip_limit, tiles_x, tiles_y), "reloc_clahe_u8: tiles_x, tiles_y must be in 1..64 and clip_limit finite");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    HostStaging st{ctx};
    uint8_t *dlut = st.slot<uint8_t>(0, (int64_t)tiles_x * tiles_y * 256), *dout = st.slot<uint8_t>(1, (int64_t)w * h);
    st.upload_rows(ctx->frame_img, gray, w, h, stride);
    ClaheFrames F = {};
    F.src[0] = ctx->frame_img; F.lut[0] = dlut; F.dst[0] = dout;
    st.run([&] { return clahe_launch(ctx->stream, F, 1, clahe_geom(w, h, clip_limit, tiles_x, tiles_y), 1, w, 0, w); });
    st.download(out, dout, (int64_t)w * h);
    return st.finish();
}

// ---- rectification entry points ----------------------------------------------------------------------------
RELOC_API int reloc_set_rectify_map(reloc_ctx *ctx, const int16_t *xy, const uint16_t *alpha, int w, int h)
{
    ARG_CHECK_CTX(ctx, true, "ctx is NULL");
    RectifyStage &r = ctx->img.rectify;
    if (!xy) {
        r.w = r.h = 0;
        return RELOC_OK;
    }
    ARG_CHECK(alpha && w >= 1 && h >= 1, "reloc_set_rectify_map: alpha is NULL or the size is not positive");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("rectification map exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    if (!r.plane) {
        // first enable, one block: the plane, then maps and depth of the largest frame
        const int64_t px = (int64_t)ctx->max_w * ctx->max_h;
        if (int rc = r.block.layout(ctx, [&](BlockCarver &c) {
                c.own(r.plane, stage_plane_bytes(ctx));
                c.aligned<64>(r.xy, px * 2);
                c.aligned<4>(r.alpha, px);
                c(r.depth, px);
            })) return rc;
    }
    // frames in flight may still read the previous map
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(r.xy, xy, (size_t)w * h * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(r.alpha, alpha, (size_t)w * h * 2, hipMemcpyHostToDevice));
    r.w = w; r.h = h;
    return RELOC_OK;
}

RELOC_API int reloc_get_rectify_map(reloc_ctx *ctx, int32_t *w, int32_t *h)
{
    ARG_CHECK_CTX(ctx, w && h, "reloc_get_rectify_map");
    *w = ctx->img.rectify.w; *h = ctx->img.rectify.h;
    return RELOC_OK;
}

// a host-pointer remap: maps into scratch 0 / 1, destination scratch 2; elem: bytes per channel value
static int remap_host(reloc_ctx *ctx, const void *src, int sstride, int channels, int elem, const int16_t *xy, const uint16_t *alpha,
                      bool nearest, const RemapGeom &g, void *out)
{
    if (g.sw > ctx->max_w || g.sh > ctx->max_h || g.dw > ctx->max_w || g.dh > ctx->max_h) { reloc_set_error("image or map exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    const int64_t px = (int64_t)g.dw * g.dh, out_bytes = px * channels * elem;
    HostStaging st{ctx};
    const int16_t *dxy = st.upload_slot(0, xy, px * 2);
    uint16_t *dal = st.slot<uint16_t>(1, px);
    uint8_t *dout = st.slot<uint8_t>(2, out_bytes);
    st.upload_rows(ctx->frame_img, src, g.sw * channels * elem, g.sh, sstride);
    if (alpha) st.upload(dal, alpha, px * 2);
    RemapFrames F = {};
    F.src[0] = ctx->frame_img; F.xy[0] = dxy; F.alpha[0] = dal; F.dst[0] = dout;
    st.run([&] { return nearest ? remap_nearest_launch(ctx->stream, F, g, channels, elem) : remap_launch(ctx->stream, F, 1, g, channels, false, 0); });
    st.download(out, dout, out_bytes);
    return st.finish();
}

RELOC_API int reloc_remap_u8(reloc_ctx *ctx, const uint8_t *src, int sw, int sh, int sstride, int channels, const int16_t *xy,
                             const uint16_t *alpha, int dw, int dh, int nearest, int border_value, uint8_t *out)
{
    ARG_CHECK_CTX(ctx, src && xy && out && (alpha || nearest) && sw >= 1 && sh >= 1 && dw >= 1 && dh >= 1 &&
                  (channels == 1 || channels == 3) && sstride >= channels * sw && border_value >= 0 && border_value <= 255,
                  "reloc_remap_u8");
    const RemapGeom g = {sw, sh, sw * channels, dw, dh, dw * channels, border_value};
    return remap_host(ctx, src, sstride, channels, 1, xy, alpha, nearest != 0, g, out);
}

RELOC_API int reloc_remap_u16(reloc_ctx *ctx, const uint16_t *src, int sw, int sh, int sstride, const int16_t *xy, int dw, int dh,
                              int border_value, uint16_t *out)
{
    ARG_CHECK_CTX(ctx, src && xy && out && sw >= 1 && sh >= 1 && dw >= 1 && dh >= 1 && sstride >= 2 * sw && border_value >= 0 &&
                  border_value <= 65535, "reloc_remap_u16");
    const RemapGeom g = {sw, sh, sw, dw, dh, dw, border_value};        // strides in elements
    return remap_host(ctx, src, sstride, 1, 2, xy, nullptr, true, g, out);
}

RELOC_API int reloc_convert_maps(reloc_ctx *ctx, const float *mapx, const float *mapy, int w, int h, int nninterpolation,
                                 int16_t *xy_out, uint16_t *alpha_out)
{
    ARG_CHECK_CTX(ctx, mapx && mapy && xy_out && alpha_out && w >= 1 && h >= 1, "reloc_convert_maps");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("map exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    const int64_t n = (int64_t)w * h;
    HostStaging st{ctx};
    u32 *dxy = st.slot<u32>(0, n);
    uint16_t *dal = st.slot<uint16_t>(1, n);
    const float *dmx = st.upload_slot(2, mapx, n), *dmy = st.upload_slot(3, mapy, n);
    st.launch(k_convert_maps, dim3((unsigned)((n + 255) / 256)), dim3(256), dmx, dmy, (int)n, nninterpolation, dxy, dal);
    st.download(xy_out, dxy, n * 4);
    st.download(alpha_out, dal, n * 2);
    return st.finish();
}

// ---- resize entry points -------------------------------------------------------------------------------------
// a host-pointer resize: table into scratch 0, destination scratch 1
static int resize_host(reloc_ctx *ctx, const void *src, int sw, int sh, int sstride, int channels, int elem, void *out, int dw, int dh,
                       double inv_x, double inv_y, int interpolation)
{
    if (sw > ctx->max_w || sh > ctx->max_h || dw > ctx->max_w || dh > ctx->max_h) { reloc_set_error("image exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    ResizePlan P;
    if (int rc = resize_plan(sw, sh, dw, dh, inv_x, inv_y, interpolation, P)) return rc;
    const int row_bytes = sw * channels * elem;
    const int64_t out_bytes = (int64_t)dw * dh * channels * elem;
    HostStaging st{ctx};
    int32_t *dtab = st.slot<int32_t>(0, (int64_t)P.tab.size() + 1);
    uint8_t *dout = st.slot<uint8_t>(1, out_bytes);
    st.upload_rows(ctx->frame_img, src, row_bytes, sh, sstride);
    // the table is pageable host memory that dies with this call: finish() has waited for the copy by then
    if (!P.tab.empty()) st.upload(dtab, P.tab.data(), (int64_t)P.tab.size() * 4);
    ResizeFrames F = {};
    F.src[0] = ctx->frame_img; F.tab[0] = dtab; F.dst[0] = dout;
    const int stride = P.kind == RESIZE_NEAREST ? sw * channels : row_bytes;      // k_resize_nearest counts strides in elements
    st.run([&] { return resize_launch(ctx->stream, F, 1, P, sw, sh, stride, dw, dh, dw * channels, channels, elem, false, 0); });
    st.download(out, dout, out_bytes);
    return st.finish();
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
    ResizeStage &r = ctx->img.resize;
    if (sw == 0 && sh == 0 && dw == 0 && dh == 0) {
        r.sw = r.sh = r.dw = r.dh = 0;
        return RELOC_OK;
    }
    ARG_CHECK(dw >= 1 && dh >= 1 && dw <= sw && dh <= sh,
              "reloc_set_resize: sizes must be all 0 (off) or 1 <= dw <= sw and 1 <= dh <= sh");
    if (sw > ctx->max_w || sh > ctx->max_h) { reloc_set_error("resize source exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    ResizePlan area, nearest;
    if (int rc = resize_plan(sw, sh, dw, dh, 0.0, 0.0, 3, area)) return rc;
    if (int rc = resize_plan(sw, sh, dw, dh, 0.0, 0.0, 0, nearest)) return rc;
    // tables of the largest frame: 3 words and at most scale + 2 alphas per destination index and axis, one offset per index
    // and axis for the depth
    const size_t area_words = 6 * ((size_t)ctx->max_w + ctx->max_h), near_words = (size_t)ctx->max_w + ctx->max_h;
    if (area.tab.size() > area_words || nearest.tab.size() > near_words) { reloc_set_error("resize tables exceed ctx capacity"); return RELOC_E_CAPACITY; }
    if (!r.plane)       // first enable, one block: the plane, then the tables and the depth plane
        if (int rc = r.block.layout(ctx, [&](BlockCarver &c) {
                c.own(r.plane, stage_plane_bytes(ctx));
                c.aligned<64>(r.tab, area_words);
                c(r.ntab, near_words);
                c.aligned<4>(r.depth, (int64_t)ctx->max_w * ctx->max_h);
            })) return rc;
    // frames in flight may still read the previous tables
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!area.tab.empty()) HIP_TRY(hipMemcpy(r.tab, area.tab.data(), area.tab.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(r.ntab, nearest.tab.data(), nearest.tab.size() * 4, hipMemcpyHostToDevice));
    r.kind = area.kind; r.isx = area.isx; r.isy = area.isy;
    r.sw = sw; r.sh = sh; r.dw = dw; r.dh = dh;
    return RELOC_OK;
}

RELOC_API int reloc_get_resize(reloc_ctx *ctx, int32_t *sw, int32_t *sh, int32_t *dw, int32_t *dh)
{
    ARG_CHECK_CTX(ctx, sw && sh && dw && dh, "reloc_get_resize");
    const ResizeStage &r = ctx->img.resize;
    *sw = r.sw; *sh = r.sh; *dw = r.dw; *dh = r.dh;
    return RELOC_OK;
}
