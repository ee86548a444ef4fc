// reloc_speckle.hip -- OpenCV's filterSpeckles on gfx950 and the speckle stage of the dense stereo pass (include/reloc_spec.h,
// "STEREO, speckle"): connected components of the 4-neighbour relation "both valid and |a - b| <= max_diff" by label
// equivalence, every pixel of a component of at most `limit` pixels removed.  A label is a raster index, label[i] <= i always,
// a root is its own label and ends up the lowest index of its component; the result does not depend on the order of the merges.
// Four launches on the context's stream, each seeing the one before at a kernel boundary:
//   k_speckle_init    a wave takes 64 columns of one row: label = the first pixel of the pixel's run of joined neighbours inside
//                     those 64 columns (one ballot, no memory traffic), -1 for an invalid pixel; size = 0.
//   k_speckle_merge   a pixel unites with its left neighbour where a run crosses a 64-column boundary, and with its upper
//                     neighbour unless that edge follows from three others (left, upper left, upper: all joined), so a
//                     surface costs one union per run and row.  Labels of other workgroups are read and written through
//                     agent-scope atomics only (L1 is per CU).  Every loop walks strictly decreasing labels: no thread waits
//                     for another's progress.
//   k_speckle_count   a wave takes SK_ROWS rows of its 64 columns: the root of every pixel (written back as its label), a
//                     lane's SK_ROWS chains walked side by side; the lanes of a row that share a root counted with one
//                     ballot, the rows of a lane that share one summed in a register, then one integer atomic add per run
//                     of rows (a whole-image component: w h / 256 adds on its word).
//   k_speckle_apply   size[label] <= limit: the pixel is removed.
// Pixels are read through a source: an int16 plane (reloc_filter_speckles) or the disparity and status planes of the dense
// pass, quantised on the fly (the stage); the same source removes a pixel.  Counts are integers: the output is the same from
// run to run.
#include "reloc_internal.h"

constexpr int SK_W = 64;              // columns of a tile: one wave
constexpr int SK_H = 4;               // rows of a tile of k_speckle_init / _merge: one per wave
constexpr int SK_ROWS = 4;            // rows a wave of k_speckle_count walks: its tile is SK_W x (SK_H * SK_ROWS)
constexpr int SK_NONE = -1;           // the label of an invalid pixel

struct SpecklePlane {                 // an int16 plane, rows of `stride` elements
    int16_t *img;
    int stride, none;
    __device__ __forceinline__ int q(int x, int y) const { return img[(size_t)y * stride + x]; }
    __device__ __forceinline__ void remove(int x, int y) const { img[(size_t)y * stride + x] = (int16_t)none; }
};

struct SpeckleStereo {                // the planes of a dense pass (dense rows of w): q = rint(16 disparity) where status is 0
    float *disp;
    uint16_t *mm;
    uint8_t *status;
    int w, none;
    __device__ __forceinline__ int q(int x, int y) const
    {
        const size_t i = (size_t)y * w + x;
        return status[i] == RELOC_STEREO_OK ? (int)(int16_t)rintf(__fmul_rn(disp[i], 16.0f)) : none;
    }
    __device__ __forceinline__ void remove(int x, int y) const
    {
        const size_t i = (size_t)y * w + x;
        status[i] = RELOC_STEREO_SPECKLE; mm[i] = 0; disp[i] = 0.f;
    }
};

__device__ __forceinline__ bool sk_joined(int a, int b, int none, int max_diff)
{
    return a != none && b != none && abs(a - b) <= max_diff;
}

__device__ __forceinline__ int sk_load(int *label, int i) { return __hip_atomic_load(label + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of i, halving the path on the way: a label only ever drops to another member of the same tree
__device__ __forceinline__ int sk_find(int *label, int i)
{
    for (;;) {
        const int p = sk_load(label, i);
        if (p == i) return i;
        const int g = sk_load(label, p);
        if (g == p) return p;
        atomicMin(label + i, g);
        i = g;                                                      // g < p < i
    }
}

// one set out of a's and b's: the higher root is hung under the lower one; where another thread got there first, its link
// stays or is replaced by the lower of the two, and the loop goes on with what it displaced -- max(a, b) drops every turn
__device__ __forceinline__ void sk_unite(int *label, int a, int b)
{
    a = sk_find(label, a); b = sk_find(label, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(label + a, b);
        if (old == a) return;
        a = sk_find(label, old); b = sk_find(label, b);
    }
}

template <typename Src>
__global__ __launch_bounds__(SK_W * SK_H) void k_speckle_init(Src src, int w, int h, int max_diff, int *__restrict__ label, int *__restrict__ size)
{
    const int lane = threadIdx.x & 63, x0 = blockIdx.x * SK_W, x = x0 + lane, y = blockIdx.y * SK_H + (threadIdx.x >> 6);
    if (y >= h) return;                                             // wave-uniform
    const bool in = x < w;
    const int v = in ? src.q(x, y) : src.none;
    const int vl = __shfl_up(v, 1);
    const bool head = lane == 0 || !sk_joined(v, vl, src.none, max_diff);
    const unsigned long long heads = __ballot(head) & (~0ull >> (63 - lane));      // the run starts at or left of this lane
    if (!in) return;
    const int i = y * w + x;
    label[i] = v != src.none ? y * w + x0 + (63 - __clzll(heads)) : SK_NONE;
    size[i] = 0;
}

template <typename Src>
__global__ __launch_bounds__(SK_W * SK_H) void k_speckle_merge(Src src, int w, int h, int max_diff, int *label)
{
    const int lane = threadIdx.x & 63, x = blockIdx.x * SK_W + lane, y = blockIdx.y * SK_H + (threadIdx.x >> 6);
    if (y >= h) return;                                             // wave-uniform
    const bool in = x < w;
    const int none = src.none;
    const int v = in ? src.q(x, y) : none;
    const int vu = in && y > 0 ? src.q(x, y - 1) : none;
    int vl = __shfl_up(v, 1), vul = __shfl_up(vu, 1);
    if (lane == 0) {
        vl = in && x > 0 ? src.q(x - 1, y) : none;
        vul = in && x > 0 && y > 0 ? src.q(x - 1, y - 1) : none;
    }
    if (!in || v == none) return;
    const int i = y * w + x;
    const bool jl = sk_joined(v, vl, none, max_diff), ju = sk_joined(v, vu, none, max_diff);
    if (jl && lane == 0) sk_unite(label, i, i - 1);
    if (ju && !(jl && sk_joined(vl, vul, none, max_diff) && sk_joined(vul, vu, none, max_diff))) sk_unite(label, i, i - w);
}

__global__ __launch_bounds__(SK_W * SK_H) void k_speckle_count(int w, int h, int *label, int *size)
{
    const int lane = threadIdx.x & 63, x = blockIdx.x * SK_W + lane, y0 = (blockIdx.y * SK_H + (threadIdx.x >> 6)) * SK_ROWS;
    const bool in = x < w;
    // the roots of the lane's SK_ROWS pixels, the chains walked side by side: a step is SK_ROWS independent loads in flight,
    // where one chain after the other would wait for every load alone.  A row below the image is a row of invalid pixels.
    int first[SK_ROWS], root[SK_ROWS];
#pragma unroll
    for (int k = 0; k < SK_ROWS; ++k) first[k] = root[k] = in && y0 + k < h ? sk_load(label, (y0 + k) * w + x) : SK_NONE;
    for (bool more = true; more;) {
        int up[SK_ROWS];
#pragma unroll
        for (int k = 0; k < SK_ROWS; ++k) up[k] = root[k] != SK_NONE ? sk_load(label, root[k]) : SK_NONE;
        more = false;
#pragma unroll
        for (int k = 0; k < SK_ROWS; ++k) { more |= up[k] != root[k]; root[k] = up[k]; }
    }
    int run_root = SK_NONE, run = 0;                                // this lane's rows so far that head a run of one root
#pragma unroll
    for (int k = 0; k < SK_ROWS; ++k) {
        const int r = root[k];
        if (r != first[k]) __hip_atomic_store(label + (y0 + k) * w + x, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int rp = __shfl_up(r, 1);
        const bool head = lane == 0 || r != rp;
        const unsigned long long above = __ballot(head) & ~(~0ull >> (63 - lane));      // the heads right of this lane
        const int len = (above ? __ffsll((long long)above) - 1 : 64) - lane;
        const int hr = head ? r : SK_NONE;
        if (hr == run_root) run += len;
        else {
            if (run_root != SK_NONE) atomicAdd(size + run_root, run);
            run_root = hr; run = len;
        }
    }
    if (run_root != SK_NONE) atomicAdd(size + run_root, run);
}

template <typename Src>
__global__ __launch_bounds__(256) void k_speckle_apply(Src src, int w, int h, int limit, const int *__restrict__ label, const int *__restrict__ size)
{
    const int x = blockIdx.x * SK_W + (threadIdx.x & 63), y = blockIdx.y * SK_H + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int r = label[y * w + x];
    if (r != SK_NONE && size[r] <= limit) src.remove(x, y);
}

// the four launches on ctx's stream; label and size: w * h words each
template <typename Src>
static int speckle_launch(reloc_ctx *ctx, const Src &src, int w, int h, int limit, int max_diff, int *label, int *size)
{
    const dim3 tiles((w + SK_W - 1) / SK_W, (h + SK_H - 1) / SK_H), block(SK_W * SK_H);
    hipLaunchKernelGGL(k_speckle_init<Src>, tiles, block, 0, ctx->stream, src, w, h, max_diff, label, size);
    hipLaunchKernelGGL(k_speckle_merge<Src>, tiles, block, 0, ctx->stream, src, w, h, max_diff, label);
    hipLaunchKernelGGL(k_speckle_count, dim3(tiles.x, (h + SK_H * SK_ROWS - 1) / (SK_H * SK_ROWS)), block, 0, ctx->stream, w, h, label, size);
    hipLaunchKernelGGL(k_speckle_apply<Src>, tiles, block, 0, ctx->stream, src, w, h, limit, label, size);
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

int stereo_speckle_launch(reloc_ctx *ctx, int w, int h)
{
    StereoState &s = ctx->stereo;
    const SpeckleStereo src = {s.dense.disp, s.dense.mm, s.dense.status, w, -16};
    // k_stereo_dense_finish was the last reader of the best plane: 8 bytes per pixel, a label and a size
    int *label = (int *)s.dense.best;
    return speckle_launch(ctx, src, w, h, s.speckle_window, 16 * s.speckle_range, label, label + (int64_t)w * h);
}

RELOC_API int reloc_filter_speckles(reloc_ctx *ctx, int16_t *img, int w, int h, int stride, int new_val, int max_speckle_size, int max_diff)
{
    ARG_CHECK_CTX(ctx, img && w >= 1 && h >= 1 && stride >= w && max_speckle_size >= 0 && max_diff >= 0 && new_val >= -32768 && new_val <= 32767,
                  "reloc_filter_speckles");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    const int64_t px = (int64_t)w * h;
    HostStaging st{ctx};
    int16_t *d = st.slot<int16_t>(0, px);
    int *label = st.slot<int>(1, px * 2);
    if (st.rc) return st.finish();
    st.upload_rows(d, img, w * 2, h, stride * 2);
    const SpecklePlane src = {d, w, new_val};
    st.run([&] { return speckle_launch(ctx, src, w, h, max_speckle_size, max_diff, label, label + px); });
    // only the w elements of a row go back: the caller's padding stays as it is
    st.run([&] { st.hip(hipMemcpy2DAsync(img, (size_t)stride * 2, d, (size_t)w * 2, (size_t)w * 2, h, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy2DAsync"); return st.rc; });
    return st.finish();
}

RELOC_API int reloc_set_stereo_speckle(reloc_ctx *ctx, int window, int range)
{
    ARG_CHECK_CTX(ctx, true, "reloc_set_stereo_speckle");
    if (window < 0) { reloc_set_error("bad argument: stereo speckle window %d is negative", window); return RELOC_E_ARG; }
    if (range < 0 || range > RELOC_STEREO_SPECKLE_RANGE_MAX) {
        reloc_set_error("bad argument: stereo speckle range %d outside 0..%d", range, RELOC_STEREO_SPECKLE_RANGE_MAX);
        return RELOC_E_ARG;
    }
    ctx->stereo.speckle_window = window;
    ctx->stereo.speckle_range = range;
    return RELOC_OK;
}

RELOC_API int reloc_get_stereo_speckle(reloc_ctx *ctx, int32_t *window, int32_t *range)
{
    ARG_CHECK(ctx, "reloc_get_stereo_speckle");
    if (window) *window = ctx->stereo.speckle_window;
    if (range) *range = ctx->stereo.speckle_range;
    return RELOC_OK;
}
