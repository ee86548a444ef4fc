// reloc_teach.h -- what the teach-side files (reloc_record, _stereo, _stereo_dense through reloc_stereo_match.h, _occupancy,
// _correlation, _route, _obstacle .hip) share and no other file includes: the ordered compaction of a 1024-thread workgroup, the
// depth pixel of the obstacle cloud, the occupancy map and the obstacle profile, the frame source and map point of the occupancy
// map and the correlation scan (host side: FrameSrc, frame_from_*, FRAME_KERNEL, frame_transform_check, occ_need_map), the
// last dense stereo pass of a context, the staging of a stereo pair from the caller's memory.
#pragma once
#include "reloc_internal.h"

// Ordered compaction, one chunk of a workgroup of 1024 threads (16 waves): the rank of this lane among the chunk's lanes with
// `keep`, in thread order, counted from `base`; total: the chunk's kept lanes, the same in every thread, so the caller keeps its
// running base in a register (base += total) and no thread has to publish it.  s_wsum: 16 ints of LDS, the helper's alone.
// Reuse of s_wsum between chunks: a fast wave must not write its next count while a slow one still sums this chunk's, which
// is what the first barrier is for; the second stands between the 16 writes and the sums.  Every thread of the workgroup calls.
__device__ __forceinline__ int block_rank(bool keep, int *s_wsum, int base, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(keep);
    __syncthreads();
    if (lane == 0) s_wsum[wave] = __popcll(bal);
    __syncthreads();
    total = 0;
    for (int w = 0; w < 16; ++w) {
        const int c = s_wsum[w];
        if (w < wave) base += c;
        total += c;
    }
    return base + __popcll(bal & ((1ull << lane) - 1ull));
}

// A depth plane on the device and the pixels a cloud takes of it: every step-th of w x h, rows `stride` pixels apart, float32
// metres or uint16 millimetres (tf_wall_clock_relay_v55.py:1020-1038).
struct DepthGrid {
    const void *data;
    int is_f32, w, h, stride, step;
    float cx, cy, fx, fy, zmin, zmax;
    __host__ __device__ int cols() const { return (w + step - 1) / step; }
    __host__ __device__ int rows() const { return (h + step - 1) / step; }
};
static inline DepthGrid depth_grid(const void *data, int is_f32, int w, int h, int stride, int step, const double K4[4], float zmin,
                                   float zmax)
{
    return DepthGrid{data, is_f32, w, h, stride, step, (float)K4[2], (float)K4[3], (float)K4[0], (float)K4[1], zmin, zmax};
}

// Pixel `at` of a depth plane in metres, float32: as it lies, or uint16 millimetres divided by 1000.  f32 is the caller's to pass
// so that a kernel templated on the format folds the branch.
__device__ __forceinline__ float depth_pixel(const void *data, bool f32, size_t at)
{
    return f32 ? reinterpret_cast<const float *>(data)[at] : __fdiv_rn((float)reinterpret_cast<const uint16_t *>(data)[at], 1000.0f);
}

// Pixel i of the grid in raster order: p = (z, -(u - cx) / fx * z, -(v - cy) / fy * z) in float32, true iff zmin < z < zmax and
// z is finite.
__device__ __forceinline__ bool depth_grid_point(const DepthGrid &g, bool f32, int i, float p[3])
{
    const int gw = g.cols(), v = (i / gw) * g.step, u = (i % gw) * g.step;
    const float z = depth_pixel(g.data, f32, (size_t)v * g.stride + u);
    p[0] = z;
    p[1] = -__fmul_rn(__fdiv_rn(__fsub_rn((float)u, g.cx), g.fx), z);
    p[2] = -__fmul_rn(__fdiv_rn(__fsub_rn((float)v, g.cy), g.fy), z);
    return z > g.zmin && z < g.zmax && isfinite(z);
}

// What a frame of the occupancy map and of the correlation scan reads: a cloud (n rows of 3 floats at pts) or the grid of a depth
// plane, as k_depth_points takes it.  A kernel is templated on the kind.
struct OccSrc { const float *pts; int n; DepthGrid grid; };
enum { OCC_SRC_POINTS = 0, OCC_SRC_DEPTH_F32 = 1, OCC_SRC_DEPTH_U16 = 2 };
struct OccT { double v[12]; };       // the 3 x 4 sensor-to-map transform, row major

template <int SRC>
__device__ __forceinline__ int occ_src_count(const OccSrc &src) { return SRC == OCC_SRC_POINTS ? src.n : src.grid.cols() * src.grid.rows(); }

// OCCUPANCY (a): row or pixel i of the source; true iff it is a point of the cloud with three finite coordinates
template <int SRC>
__device__ __forceinline__ bool occ_src_point(const OccSrc &src, int i, float p[3])
{
    bool fin;
    if (SRC == OCC_SRC_POINTS) {
        for (int k = 0; k < 3; ++k) p[k] = src.pts[(size_t)3 * i + k];
        fin = true;
    } else fin = depth_grid_point(src.grid, SRC == OCC_SRC_DEPTH_F32, i, p);
    return fin && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

// OCCUPANCY (b): row k of the transform applied to p, float64, this order, no contraction
__device__ __forceinline__ double occ_map_coord(const OccT &T, int k, const float p[3])
{
    const double x = p[0], y = p[1], z = p[2];
    return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(T.v[4 * k], x), __dmul_rn(T.v[4 * k + 1], y)), __dmul_rn(T.v[4 * k + 2], z)), T.v[4 * k + 3]);
}

// OCCUPANCY (d): q = (x - origin) / res in double, in the grid iff -1 < q < n (trunc toward zero puts (-1, 0) into cell 0)
__device__ __forceinline__ bool occ_cell(double x, double origin, double res, int n, int &cell)
{
    const double q = __ddiv_rn(__dsub_rn(x, origin), res);
    const bool in = q > -1.0 && q < (double)n;
    cell = in ? (int)q : 0;
    return in;
}

static inline bool occ_finite(double v) { return v - v == 0.0; }

// Where a frame comes from (host): the source and its OCC_SRC_* kind on an entry point's staging, clouds and depth images through
// scratch slot 5.  A source that cannot be had leaves its code in st.rc and its text in the error: all behind it is a no-op.
struct FrameSrc { OccSrc src; int kind; };
#define FRAME_KERNEL(kern, kind) /* the instantiation of a kernel template <int SRC> for a kind */ \
    ((kind) == OCC_SRC_POINTS ? kern<OCC_SRC_POINTS> : (kind) == OCC_SRC_DEPTH_F32 ? kern<OCC_SRC_DEPTH_F32> : kern<OCC_SRC_DEPTH_U16>)

static inline FrameSrc frame_from_cloud(HostStaging &st, const float *pts, int n) { return {{n > 0 ? st.upload_slot(5, pts, (int64_t)n * 3) : nullptr, n, {}}, OCC_SRC_POINTS}; }
static inline FrameSrc frame_from_depth(HostStaging &st, const void *depth, int is_f32, int w, int h, int step, const double K4[4], float zmin, float zmax)
{
    if (!st.rc && (int64_t)w * h > (int64_t)st.ctx->max_w * st.ctx->max_h) { reloc_set_error("depth image exceeds ctx capacity"); st.rc = RELOC_E_CAPACITY; }
    const void *ddepth = st.upload_slot(5, (const uint8_t *)depth, (int64_t)w * h * (is_f32 ? 4 : 2));
    return {{nullptr, 0, depth_grid(ddepth, is_f32, w, h, w, step, K4, zmin, zmax)}, is_f32 ? OCC_SRC_DEPTH_F32 : OCC_SRC_DEPTH_U16};
}
// the last dense stereo pass of a context (its planes, w x h), or NULL: none yet
static inline const StereoState::Dense *stereo_last_dense(const reloc_ctx *ctx)
{
    const StereoState::Dense &d = ctx->stereo.dense;
    return d.block.p && d.w != 0 ? &d : nullptr;
}
// the millimetre plane of the context's last dense stereo pass where it lies, under the context's camera
static inline FrameSrc frame_from_stereo(HostStaging &st, int step, float zmin, float zmax)
{
    const StereoState::Dense *d = stereo_last_dense(st.ctx);
    if (!d) {       // an empty plane, with the caller's step: the host divides by it (cols, rows) before st.rc stops the launches
        if (!st.rc) { reloc_set_error("no dense stereo pass on this context yet"); st.rc = RELOC_E_STATE; }
        return {{nullptr, 0, depth_grid(nullptr, 0, 0, 0, 0, step, st.ctx->cam.K4, zmin, zmax)}, OCC_SRC_DEPTH_U16};
    }
    return {{nullptr, 0, depth_grid(d->mm, 0, d->w, d->h, d->w, step, st.ctx->cam.K4, zmin, zmax)}, OCC_SRC_DEPTH_U16};
}
// the 3 x 4 transform of a frame: every value finite
static inline int frame_transform_check(const double *T12, const char *who)
{
    for (int k = 0; k < 12; ++k)
        if (!occ_finite(T12[k])) { reloc_set_error("bad argument: %s: the transform must be finite", who); return RELOC_E_ARG; }
    return RELOC_OK;
}
// what reads the context's occupancy grid, the *_from_occ calls included (its plane and geometry are ctx->occ's)
static inline int occ_need_map(const reloc_ctx *ctx, const char *who) { return need_map(ctx->occ.on(), who, "occupancy", "reloc_occ_configure"); }

// What an entry point checks of a stereo pair before it enqueues anything.
static inline int stereo_pair_entry(const reloc_ctx *ctx, const reloc_ctx *right, int w, int h)
{
    if (!ctx->stereo.on()) { reloc_set_error("stereo is off on this context (reloc_set_stereo)"); return RELOC_E_STATE; }
    if (right == ctx) { reloc_set_error("bad argument: the right eye needs a context of its own"); return RELOC_E_ARG; }
    if (w > ctx->max_w || h > ctx->max_h || w > right->max_w || h > right->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    return RELOC_OK;
}

// HostStaging for a stereo pair in the caller's memory: the left frame goes to ctx->frame_img on ctx's stream, the right one to
// right->frame_img on right's stream, where its chain runs (stereo_frame, stereo_dense_frame).  After an error the two streams
// may not be ordered, so finish() waits for the right stream as well whenever that copy was enqueued: nothing of the caller's
// right frame stays in flight.
struct StereoPairStaging : HostStaging {
    reloc_ctx *right;
    bool right_busy = false;
    StereoPairStaging(reloc_ctx *c, reloc_ctx *r) : HostStaging{c}, right(r) {}
    void upload_pair(const uint8_t *img, const uint8_t *img_right, int w, int h)
    {
        upload(ctx->frame_img, img, (int64_t)w * h * image_chain_frame_bpp(ctx));
        run([&] {
            right_busy = true;
            HIP_TRY(hipMemcpyAsync(right->frame_img, img_right, (size_t)w * h * image_chain_frame_bpp(right), hipMemcpyHostToDevice, right->stream));
            return (int)RELOC_OK;
        });
    }
    int finish()
    {
        const int r = HostStaging::finish();
        if (right_busy) (void)hipStreamSynchronize(right->stream);
        right_busy = false;
        return r;
    }
};
