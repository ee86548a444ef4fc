// reloc_internal.h -- shared declarations of libreloc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/reloc.h"
#include "../../include/reloc_spec.h"
#include "reloc_block_layout.h"
#include "reloc_orb_plan.h"

#define RELOC_API extern "C" __attribute__((visibility("default")))
#define RELOC_PROF_RING 256      /* event pairs per stopwatch before reloc_prof_begin has to wait for the device */

void reloc_set_error(const char *fmt, ...);

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            reloc_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                            __LINE__);                                                     \
            return RELOC_E_HIP;                                                            \
        }                                                                                  \
    } while (0)

#define ARG_CHECK(cond, msg)                                 \
    do {                                                     \
        if (!(cond)) {                                       \
            reloc_set_error("bad argument: %s", msg);        \
            return RELOC_E_ARG;                              \
        }                                                    \
    } while (0)

// argument check of an entry point that takes a ctx: also makes the ctx's device current, so one process
// may drive several GPUs through several ctxs
#define ARG_CHECK_CTX(c, cond, msg)                           \
    do {                                                      \
        if (!(c) || !(cond)) {                                \
            reloc_set_error("bad argument: %s", msg);         \
            return RELOC_E_ARG;                               \
        }                                                     \
        (void)hipSetDevice((c)->device);                      \
    } while (0)

constexpr int MAX_REC_ROWS = 4096;   // largest record (teach rows) the fused scan accepts
constexpr int MAX_CAND = 32;         // PnP candidates per tick (5 local / 25 global)
constexpr int MAX_HYP = 1024;        // RANSAC hypotheses per candidate (iterationsCount)
constexpr int64_t MAX_DB_RECORDS = 0xFFFFF;   // the local-candidate key keeps the record index in 20 bits

// Wave issue priority of the tick's small kernels (s_setprio 3; the default, and the scan's, is 0).  With several streams
// on the chip a SIMD holds four scan waves and a wave or two of some other stream's ORB / ranking / PnP kernel; those
// kernels are short dependent chains, and at equal priority they get one issue slot in five, so every stream's non-scan
// phase stretches 2-3x (k_pyramid 49 vs 17 us, k_fast_blur 46 vs 16) and the scans of the streams overlap less.  With
// priority the same instructions are issued, only sooner: 4-stream run 6060 -> 6250 frames/s, single-stream ticks unchanged.
// -DRELOC_SMALL_PRIO=0 switches it off (A/B builds).
// Register budget of the scan kernels (k_db_scan, k_db_scan_batch, k_db_scan_emit, k_db_scan_emit_batch), capped with amdgpu_num_vgpr (0 = the compiler's choice: 112).
// Four scan waves per SIMD at 112 registers leave 64 of the 512 per lane to whatever else wants to run beside them -- and
// k_pyramid (94), k_pnp_hyp (94), k_tick_finalize (80) do not fit into 64: they wait for a scan workgroup to retire.  At 104
// (28 bytes of scratch) four scan waves leave 96 and a fifth still does not fit (5 x 104 > 512); at 96 a fifth does, and
// nothing else any more.  4-stream run, interleaved on one box (profiles/r4_scan_vgpr.log): 112 / 104 / 96 registers = 6 648 /
// 6 716 / 6 560 frames/s, synchronous whole-database tick 273 / 269 / 280 us.  (Cutting k_pnp_finish and the emit pass to 96 registers so
// that they fit beside the scans as well: nothing with three scan generations, 6 747-6 760 vs 6 753 frames/s; with the one generation of
// today 4-7 % WORSE, 6 320-6 550 vs 6 822 -- they are better off in the gap between two scans than competing with one; same log.)
#ifndef RELOC_SCAN_NUM_VGPR
#define RELOC_SCAN_NUM_VGPR 104
#endif
#if RELOC_SCAN_NUM_VGPR > 0
// (the backend doubles the attribute's value on targets with the unified VGPR / AGPR file: half of the wanted count is passed)
#define RELOC_SCAN_VGPR_ATTR __attribute__((amdgpu_num_vgpr(RELOC_SCAN_NUM_VGPR / 2)))
#else
#define RELOC_SCAN_VGPR_ATTR
#endif
#ifndef RELOC_SMALL_PRIO
#define RELOC_SMALL_PRIO 3
#endif
#define RELOC_SMALL_KERNEL_PRIO() __builtin_amdgcn_s_setprio(RELOC_SMALL_PRIO)

// Result record of one tick (device resident, copied out by reloc_tick_result)
struct TickResult {
    double anchor_pose[7];
    double reproj;
    int32_t n_inl;
    int32_t lm_idx;
    int32_t outcome;
    int32_t n_candidates;
    int32_t n_features;
    int32_t relocating;   // candidates came from the whole-database search (G:344)
    int32_t pad[2];       // 96 bytes; pad[0] of a record in HOST memory: the tick's sequence stamp, stored last (reloc_tick_wait)
};
static_assert(sizeof(TickResult) == 96, "TickResult is the 96-byte record documented in include/reloc.h");
// the same offsets as the TICK_RESULT dtype of engine.py, which is how Python reads a record
static_assert(offsetof(TickResult, anchor_pose) == 0 && offsetof(TickResult, reproj) == 56, "TickResult layout");
static_assert(offsetof(TickResult, n_inl) == 64 && offsetof(TickResult, lm_idx) == 68 && offsetof(TickResult, outcome) == 72,
              "TickResult layout");
static_assert(offsetof(TickResult, n_candidates) == 76 && offsetof(TickResult, n_features) == 80 &&
              offsetof(TickResult, relocating) == 84 && offsetof(TickResult, pad) == 88, "TickResult layout");

// what reloc_tick_accumulate_dev left behind (device resident)
struct AccumResult {
    double nearest_m;     // distance to the nearest filed record (-1: not evaluated)
    int32_t appended;     // 1: a record was written behind the arena's last one
    int32_t n_kpts;       // keypoints with valid depth
};

// One resident landmark database: structure of arrays with reserved capacity (rows: cap_rows, records: cap_records).
// The six database arrays of one arena (desc, pts3d, kp2d, off, pose, xy_heading) are held by reference count: the
// context that uploaded them and every context that adopted them with reloc_db_share hold one reference each, and the
// arrays are freed by whoever lets go last.  An owner that re-allocates (growth past the reserve, a new upload) or is
// destroyed therefore never frees memory an adopter still scans: the adopter keeps the arrays -- and the record count --
// it adopted until it calls reloc_db_share / reloc_db_upload again.
// The arena is the unit of ownership: everything a context knows about a database is in its DbArena, a finished arena
// enters a slot by assignment and leaves it through db_arena_release (reloc_db.hip), nothing else frees database memory.
struct DbShare { int refs = 1; };

struct DbArena {
    DbShare *share = nullptr;         // reference count of the six shared arrays
    bool shared = false;              // the arrays were adopted from another ctx (reloc_db_share): read-only here
    int64_t cap_records = 0, cap_rows = 0;
    int64_t records = 0, rows = 0;
    int max_rows = 0;
    uint8_t *desc = nullptr;          // cap_rows x 32
    float *pts3d = nullptr;           // cap_rows x 3
    float *kp2d = nullptr;            // cap_rows x 2 (keypoints_2d; only kept for reloc_db_fetch)
    int64_t *off = nullptr;           // cap_records + 1
    double *pose = nullptr;           // cap_records x 7
    double *xy_heading = nullptr;     // cap_records x 4 (x, y, cos heading, sin heading) for candidate selection
    int32_t *counts = nullptr;        // cap_records per-record mutual counts; this holder's own, like topk_part
    unsigned long long *topk_part = nullptr;   // per-block winners of the two-stage top-k (topk_blocks x 32)
    int topk_blocks = 0;
};

// Per-candidate PnP output
struct PnpOut {
    double Rt[12];       // refined pose (teach cam -> current cam)
    double rvec[3];
    double reproj_mean;  // mean inlier reprojection error (px) under the refined pose
    int32_t ok;
    int32_t n_inl;
    int32_t best_h;
    int32_t n_matches;
};

// ---- wave-wide reductions in the VALU's DPP network -------------------------------------------------
// quad_perm / mirror steps leave a row's result in all of its 16 lanes, row_bcast15 / row_bcast31 carry it
// across the four rows, lane 63 ends with the total.  A chain of such reductions costs a few VALU
// instructions each instead of six dependent ds_bpermute round trips.  All 64 lanes must be active.
template <bool MAX>      // the wave's maximum (MAX) or minimum
__device__ __forceinline__ unsigned wave_minmax_u32(unsigned v)
{
    int x = (int)v;
#define RELOC_DPP_STEP(ctrl, rmask)                                                                     \
    {                                                                                                   \
        const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(x, x, ctrl, rmask, 0xF, false);         \
        x = (int)((MAX ? (unsigned)x > o : (unsigned)x < o) ? (unsigned)x : o);                          \
    }
    RELOC_DPP_STEP(0xB1, 0xF)    // quad_perm [1,0,3,2]
    RELOC_DPP_STEP(0x4E, 0xF)    // quad_perm [2,3,0,1]
    RELOC_DPP_STEP(0x141, 0xF)   // row_half_mirror
    RELOC_DPP_STEP(0x140, 0xF)   // row_mirror
    RELOC_DPP_STEP(0x142, 0xA)   // row_bcast15 -> rows 1, 3
    RELOC_DPP_STEP(0x143, 0xC)   // row_bcast31 -> rows 2, 3
#undef RELOC_DPP_STEP
    return (unsigned)__builtin_amdgcn_readlane(x, 63);
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) { return wave_minmax_u32<true>(v); }
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) { return wave_minmax_u32<false>(v); }

// value of lane (l ^ K) for K = 1, 2, 4, 8 through DPP (quad permutes, row shifts with bank masks, row rotate)
template <int K>
__device__ __forceinline__ unsigned dpp_xor(unsigned v)
{
    static_assert(K == 1 || K == 2 || K == 4 || K == 8, "in-row exchanges only");
    const int x = (int)v;
    if constexpr (K == 1) return (unsigned)__builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false);
    else if constexpr (K == 2) return (unsigned)__builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false);
    else if constexpr (K == 8) return (unsigned)__builtin_amdgcn_update_dpp(x, x, 0x128, 0xF, 0xF, false);
    else {
        const int t = __builtin_amdgcn_update_dpp(x, x, 0x104, 0xF, 0x5, false);      // banks 0, 2 <- lane + 4
        return (unsigned)__builtin_amdgcn_update_dpp(t, x, 0x114, 0xF, 0xA, false);    // banks 1, 3 <- lane - 4
    }
}

// integer sum (exact in any order); every lane gets the total
__device__ __forceinline__ int wave_sum_i32(int x)
{
#define RELOC_DPP_STEP(ctrl, rmask) x += __builtin_amdgcn_update_dpp(0, x, ctrl, rmask, 0xF, false);
    RELOC_DPP_STEP(0xB1, 0xF)
    RELOC_DPP_STEP(0x4E, 0xF)
    RELOC_DPP_STEP(0x141, 0xF)
    RELOC_DPP_STEP(0x140, 0xF)
    RELOC_DPP_STEP(0x142, 0xA)
    RELOC_DPP_STEP(0x143, 0xC)
#undef RELOC_DPP_STEP
    return __builtin_amdgcn_readlane(x, 63);
}

// ---- heading test shared by the scan and the candidate kernels (M:296-301, G:329-330) --------------
__device__ __forceinline__ void quat_to_rot(double qx, double qy, double qz, double qw, double R[9])
{
    R[0] = 1 - 2 * (qy * qy + qz * qz); R[1] = 2 * (qx * qy - qz * qw);     R[2] = 2 * (qx * qz + qy * qw);
    R[3] = 2 * (qx * qy + qz * qw);     R[4] = 1 - 2 * (qx * qx + qz * qz); R[5] = 2 * (qy * qz - qx * qw);
    R[6] = 2 * (qx * qz - qy * qw);     R[7] = 2 * (qy * qz + qx * qw);     R[8] = 1 - 2 * (qx * qx + qy * qy);
}

// |wrap(teach_hdg - cur_hdg)| < tol  <=>  cos(teach_hdg - cur_hdg) > cos(tol); the database index keeps
// (cos, sin) of every record's heading, so the test is one dot product.
__device__ __forceinline__ bool heading_ok(const double *__restrict__ rec4, double cc, double sc, double cos_tol)
{
    return rec4[2] * cc + rec4[3] * sc > cos_tol;
}

// (cos, sin) of the robot's heading from the base_link quaternion (x, y, z, w)
__device__ __forceinline__ void cur_heading_q(const double q[4], double &cc, double &sc)
{
    double Rb[9];
    quat_to_rot(q[0], q[1], q[2], q[3], Rb);
    const double n = sqrt(Rb[0] * Rb[0] + Rb[3] * Rb[3]);       // fwd = (R00, R10); only the direction matters
    cc = n > 0 ? Rb[0] / n : 1.0;
    sc = n > 0 ? Rb[3] / n : 0.0;
}

// Lens distortion k1 k2 p1 p2 k3 (include/reloc_spec.h): passed by value to both instantiations of a DIST-templated
// kernel; the pinhole one (DIST = false) never reads it, so its code is that of a kernel without the argument.  Operation
// order as cv::projectPoints / cv::undistortPoints (no FMA: the library builds with -ffp-contract=off), so
// tests/distortion_ref.py restates it bit for bit.
struct DistCoef { double k1, k2, p1, p2, k3; };
struct CamK4 { double v[4]; };         // fx fy cx cy by value
// host side: d = k1 k2 p1 p2 k3, or NULL for all zeros
static inline DistCoef make_dist(const double *d)
{
    return d ? DistCoef{d[0], d[1], d[2], d[3], d[4]} : DistCoef{};
}
// host side: n coefficients all finite (x - x is NaN for an infinity or a NaN)
static inline bool dist_finite(const double *d, int n = 5)
{
    if (!d) return true;
    for (int k = 0; k < n; ++k) if (!(d[k] - d[k] == 0.0)) return false;
    return true;
}
// normalized (x, y) -> distorted normalized (xd, yd)
__device__ __forceinline__ void distort_norm(const DistCoef &d, double x, double y, double &xd, double &yd)
{
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double rad = 1.0 + d.k1 * r2 + d.k2 * r4 + d.k3 * r6;
    const double a1 = 2.0 * x * y, a2 = r2 + 2.0 * x * x, a3 = r2 + 2.0 * y * y;
    xd = x * rad + d.p1 * a1 + d.p2 * a2;
    yd = y * rad + d.p1 * a3 + d.p2 * a1;
}
// pixel (u, v) -> undistorted normalized (x, y): RELOC_UNDISTORT_ITERS fixed-point steps
__device__ __forceinline__ void undistort_norm(const DistCoef &d, const double K4[4], double u, double v, double &x, double &y)
{
    const double x0 = (u - K4[2]) * (1.0 / K4[0]), y0 = (v - K4[3]) * (1.0 / K4[1]);
    x = x0; y = y0;
    for (int it = 0; it < RELOC_UNDISTORT_ITERS; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((d.k3 * r2 + d.k2) * r2 + d.k1) * r2);
        if (icdist < 0) { x = x0; y = y0; break; }
        const double dx = 2.0 * d.p1 * x * y + d.p2 * (r2 + 2.0 * x * x);
        const double dy = d.p1 * (r2 + 2.0 * y * y) + 2.0 * d.p2 * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
}

// What a whole-database counting scan (launch_db_count, k_db_scan_batch) may leave out.  The heading mask: records whose
// teach heading is incompatible with the robot's are not scored (count 0), exactly the records the reference skips at
// G:329-330; xyh == NULL: no mask.  skip_if: the scan of a frame that needs none.
struct ScanMask {
    const double *xyh = nullptr;
    double q[4] = {0, 0, 0, 1};                  // base_link quaternion x y z w of the robot
    double cos_tol = 6.123233995736766e-17;      // cos(HEADING_TOL_DEG = 90 degrees) in double
    const int32_t *skip_if = nullptr;            // RELOC_TICK_AUTO: the whole launch stands down when *skip_if != 0
};

// ---- context state ("Context state") ------------------------------------------------------------------------
// Device memory: every block of a context is a DevBlock member of the state that uses it (one per lifetime, laid out by one
// carve list in the state's file) and goes with the context; a DbArena owns its database.  Settings: one struct per image
// stage and one for the camera, next to the buffers they fill.  on(): the stage runs.  same(): two contexts may share a
// batched launch; it compares every setting of its struct and no buffer, and nothing else decides that (ctx_batch_check,
// image_chain_check*): a new setting is compared because it is a member of its stage.

// A device block that a context owns: grown when too small, never shrunk, freed with its owner (move-only).  Its layout is a
// list of carve lines in block order (BlockCarver, reloc_block_layout.h) that layout() walks twice: for the size, writing
// nothing, then behind reserve() for the pointers.  A failed reserve() or layout() leaves the block, its size and every pointer
// carved from it as they were.
struct DevBlock {
    uint8_t *p = nullptr;
    size_t bytes = 0;
    DevBlock() = default;
    DevBlock(DevBlock &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBlock &operator=(DevBlock &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBlock() { release(); }
    // Replaces a missing or smaller block: the new one is allocated first, then, behind a drain of ctx's stream (work in flight
    // may still use the old one), the first `keep` bytes move over and the old one is freed (reloc_ctx.hip)
    int reserve(reloc_ctx *ctx, size_t need, size_t keep = 0);
    template <typename Fn>      // lines(BlockCarver &): the carve lines
    int layout(reloc_ctx *ctx, Fn lines, size_t keep = 0)
    {
        BlockCarver size;
        lines(size);
        if (int rc = reserve(ctx, size.at, keep)) return rc;
        BlockCarver commit{p};
        lines(commit);
        return RELOC_OK;
    }
private:
    void release();
};

// camera (reference M:49-52, M:107-112) and lens (reloc_set_camera, reloc_set_distortion)
struct CameraModel {
    double K4[4] = {RELOC_FX, RELOC_FY, RELOC_CX, RELOC_CY};
    double b2c_t[3] = {0.35, 0.0, 0.18};
    double b2c_R[9] = {0, -1, 0, 0, 0, -1, 1, 0, 0};
    double dist[5] = {0, 0, 0, 0, 0};   // k1 k2 p1 p2 k3; zeros normalised to +0, so equal models compare equal byte for byte
    bool has_dist = false;               // a coefficient is non-zero: the DIST kernels run
    const double *lens() const { return has_dist ? dist : nullptr; }      // NULL = pinhole kernels (make_dist: all zeros)
    bool same(const CameraModel &o) const
    {
        return memcmp(K4, o.K4, sizeof(K4)) == 0 && memcmp(b2c_t, o.b2c_t, sizeof(b2c_t)) == 0 &&
               memcmp(b2c_R, o.b2c_R, sizeof(b2c_R)) == 0 && memcmp(dist, o.dist, sizeof(dist)) == 0;
    }
};

// Bayer stage in front of the whole image chain (reloc_set_bayer): every frame of the chain's entry points is a raw 8-bit mosaic
struct BayerStage {
    int code = 0;                        // RELOC_BAYER_*2BGR; 0 = off, the default
    DevBlock block;                      // taken on the first enable
    uint8_t *plane = nullptr;            // demosaiced gray plane, row stride (w + 63) & ~63
    bool on() const { return code != 0; }
    bool same(const BayerStage &o) const { return code == o.code; }
};

// Pixel format of the frames of the chain's entry points (reloc_set_pixel_format); RELOC_FMT_BGR = the 3-channel frames, the
// default.  MONO8 frames are gray planes and enter the chain as they are; the packed formats (BGRA, RGBA, YUYV, UYVY) take
// the head-of-chain stage k_unpack, in the Bayer stage's place (the two exclude each other)
struct PixfmtStage {
    int fmt = RELOC_FMT_BGR;
    DevBlock block;                      // taken on the first enable of a packed format
    uint8_t *plane = nullptr;            // unpacked gray plane of a packed format, row stride (w + 63) & ~63
    bool on() const { return fmt >= RELOC_FMT_BGRA; }                    // the unpack stage runs
    int bpp() const { return fmt == RELOC_FMT_BGR ? 3 : fmt == RELOC_FMT_MONO8 ? 1 : fmt <= RELOC_FMT_RGBA ? 4 : 2; }
    bool yuv422() const { return fmt == RELOC_FMT_YUYV || fmt == RELOC_FMT_UYVY; }
    bool same(const PixfmtStage &o) const { return fmt == o.fmt; }
};

// downscale stage at the head of the image chain on 3-channel frames (reloc_set_resize); all 0 = off, the default
struct ResizeStage {
    int sw = 0, sh = 0;                  // the size every frame must have
    int dw = 0, dh = 0;                  // the working frame: what rectification, CLAHE, ORB, the recorder and the camera see
    int kind = 0, isx = 1, isy = 1;      // kernel kind and integer box of the INTER_AREA resize (reloc_image.hip): derived from the sizes
    DevBlock block;                      // taken on the first enable; the pointers below lie in it
    int32_t *tab = nullptr;              // INTER_AREA tap lists
    int32_t *ntab = nullptr;             // INTER_NEAREST offsets of the depth image
    uint8_t *plane = nullptr;            // resized gray plane, row stride (dw + 63) & ~63
    uint16_t *depth = nullptr;           // resized depth (nearest), dense rows of dw
    bool on() const { return dw > 0; }
    bool same(const ResizeStage &o) const { return sw == o.sw && sh == o.sh && dw == o.dw && dh == o.dh; }
};

// rectification in front of ORB and CLAHE on 3-channel frames (reloc_set_rectify_map); 0 x 0 = off, the default
struct RectifyStage {
    int w = 0, h = 0;                    // map = frame size
    DevBlock block;                      // taken on the first enable; the pointers below lie in it
    int16_t *xy = nullptr;               // max_h x max_w x 2, dense rows of w
    uint16_t *alpha = nullptr;           // max_h x max_w
    uint8_t *plane = nullptr;            // rectified gray plane, row stride (w + 63) & ~63
    uint16_t *depth = nullptr;           // rectified depth (nearest), dense rows of w
    bool on() const { return w > 0; }
    bool same(const RectifyStage &o) const { return w == o.w && h == o.h; }      // the maps themselves may differ per context
};

// CLAHE in front of ORB on 3-channel frames (reloc_set_clahe); tiles 0 x 0 = off, the default
struct ClaheStage {
    double clip = 0.0;                   // clipLimit (0 when off; -0 normalised to +0)
    int tx = 0, ty = 0;                  // tileGridSize
    DevBlock block;                      // taken on the first enable; the pointers below lie in it
    uint8_t *plane = nullptr;            // equalised gray plane, row stride (w + 63) & ~63
    uint8_t *lut = nullptr;              // tiles_y x tiles_x x 256 LUTs (64 x 64 x 256 bytes)
    bool on() const { return tx > 0; }
    bool same(const ClaheStage &o) const { return tx == o.tx && ty == o.ty && clip == o.clip; }
};

// ORB's detection mask on the working frame of the image chain (reloc_set_orb_mask); 0 x 0 = off, the default
struct OrbMaskStage {
    int w = 0, h = 0;                    // the persistent mask = working-frame size
    DevBlock block;                      // both pyramids, taken on the first use of a mask; grows with the arenas (orb_grow)
    uint8_t *pyr = nullptr;              // its mask pyramid, geometry of orb.buf.pyr; level 0 is the mask as given
    uint8_t *call = nullptr;             // the same for the mask of one reloc_orb_detect_compute_masked call
    bool built = false;                  // levels 1.. of pyr belong to the mask of level 0 (k_mask_level ran since it was set)
    OrbParams built_prm;                 // ... on the level geometry of these ORB parameters
    const uint8_t *last = nullptr;       // the pyramid the last masked frame used, of last_w x last_h (reloc_orb_mask_level)
    int last_w = 0, last_h = 0;
    bool on() const { return w > 0; }
    bool same(const OrbMaskStage &o) const { return w == o.w && h == o.h; }      // the masks themselves may differ per context
};

// Match policy of the tick (reloc_set_match_policy; include/reloc_spec.h "MATCH POLICY"): the two places it decides are
// scan_counts() and launch_tick_emit()
struct MatchPolicy {
    int policy = RELOC_MATCH_CROSS;
    double ratio = RELOC_LOWE_RATIO;     // stored and ignored under RELOC_MATCH_CROSS
    bool ratio_on() const { return policy == RELOC_MATCH_RATIO; }
    bool same(const MatchPolicy &o) const { return policy == o.policy && ratio == o.ratio; }
};

// Sparse stereo depth of a context, the left eye's (reloc_set_stereo; include/reloc_spec.h "STEREO"); baseline 0 = off, the
// default.  The buffers and the two events are taken on the first enable (reloc_stereo.hip).
struct StereoState {
    double baseline = 0.0;               // metres
    int min_disp = 0, num_disp = RELOC_STEREO_NUM_DISP_DEFAULT, uniq = RELOC_STEREO_UNIQUENESS_DEFAULT, lr = 1;
    DevBlock block;                      // taken on the first enable; the four pointers below lie in it (stereo_sparse_lines)
    uint8_t *plane = nullptr;            // right eye's gray plane where its chain has no stage on (dense rows)
    uint16_t *mm = nullptr;              // max_feat: depth of the keypoints of the frame's ORB output
    float *disp = nullptr;               // max_feat
    uint8_t *status = nullptr;           // max_feat
    hipEvent_t right_done = nullptr;     // the right eye's chain has written its plane (recorded on the right context's stream)
    hipEvent_t left_ready = nullptr;     // this context's stream so far: the right frame's copy, the last stereo kernel (which
                                         // reads the right chain's planes); the next right chain waits for it
    bool ran = false;                    // a stereo pass was enqueued: mm / disp / status belong to a frame (reloc_stereo_debug)
    // Dense stereo depth ("STEREO, dense"): one block of max_w x max_h pixels, taken on the first dense call of the context
    // (stereo_dense_alloc); a context that never asks for a dense plane has none of it.
    struct Dense {
        DevBlock block;                  // the pointers below lie in it (stereo_dense_lines)
        uint32_t *rmap = nullptr;        // the right disparity map as cost << 11 | d' keys, KEY_NONE = no candidate
        uint2 *best = nullptr;           // per pixel d* | C(d*) << 16, C(d* - 1) | C(d* + 1) << 16: k_stereo_dense to k_stereo_dense_finish
        float *disp = nullptr;
        uint16_t *mm = nullptr;
        uint8_t *status = nullptr;
        uint8_t *left = nullptr;         // left eye's gray plane where its chain has no stage on (dense rows)
        int w = 0, h = 0;                // the last dense pass (reloc_stereo_dense_debug); 0 = none yet
    } dense;
    // The speckle stage behind the dense pass ("STEREO, speckle"; reloc_set_stereo_speckle, a setting of its own): window 0 = off,
    // the default.  It labels in the dense block's best plane, which k_stereo_dense_finish has read by then: no memory of its own.
    int speckle_window = 0, speckle_range = 1;
    // Semi-global aggregation in the dense pass ("STEREO, semi-global"; reloc_set_stereo_sgm, a setting of its own): paths 0 = off,
    // the default, else 4 or 8.  The volumes are taken at the first semi-global pass of the context and sized from that pass
    // (stereo_sgm_alloc); they grow when a later pass needs more.  A context that never turns it on has none of it.
    int sgm_paths = 0, sgm_p1 = RELOC_STEREO_SGM_P1_DEFAULT, sgm_p2 = RELOC_STEREO_SGM_P2_DEFAULT;
    struct Sgm {
        DevBlock block;                  // the pointers below lie in it (stereo_sgm_lines)
        uint16_t *vol = nullptr;         // C as [v][u][k], k = d - min_disparity; 0xFFFF outside D(u)
        uint32_t *sum = nullptr;         // S, the same layout
        uint4 *best = nullptr;           // per pixel d*, S(d*), S(d* - 1), S(d* + 1): k_sgm_select to k_stereo_dense_finish
        int64_t cap_entries = 0, cap_px = 0;      // what vol / sum and best hold
        int w = 0, h = 0, nd = 0, dmin = 0;       // the last semi-global pass (reloc_stereo_sgm_debug); w 0 = none yet
    } sgm;
    // The data term of the three matchers ("STEREO, census"; reloc_set_stereo_cost, a setting of its own): SAD, the default, or
    // the census.  The census planes of a pass's two eyes (dense rows of the pass's width) are taken on the first census pass
    // (stereo_census_alloc); a context that never selects the census has none of it.
    int cost = RELOC_STEREO_COST_SAD;
    struct Census {
        DevBlock block;                  // the pointers below lie in it (stereo_census_lines)
        uint8_t *left = nullptr, *right = nullptr;
    } census;
    bool on() const { return baseline > 0.0; }
};

// Teach-time occupancy map of a context (reloc_occ_configure; include/reloc_spec.h "OCCUPANCY"; reloc_occupancy.hip); 0 x 0 = none,
// the default: a context that never configures a map allocates and launches nothing of it.
struct OccState {
    int w = 0, h = 0;                    // cells
    int sub = RELOC_OCC_SUBSAMPLE_DEFAULT;
    double ox = 0, oy = 0, res = 0, z_lo = 0, z_hi = 0;
    DevBlock block;                      // the pointers below lie in it
    int32_t *acc = nullptr;              // w * h: sums of the cells beyond the on-chip window, zero between frames
    int64_t *counters = nullptr;         // frames_integrated, total_points_integrated, frames_skipped_empty
    int32_t *frame = nullptr;            // the last frame: rays, box of its far rays
    int8_t *units = nullptr;             // w * h: the grid, log-odds in units of 0.2, row 0 at origin_y
    uint8_t *pgm = nullptr;              // w * h: the classified plane of the last reloc_occ_read
    bool on() const { return w > 0; }
};

// Depth-correlation anchor of a context (include/reloc_spec.h "CORRELATION"; reloc_correlation.hip); 0 x 0 = no map, the default: a
// context that never sets a correlation map allocates and launches nothing of it.  Two blocks: the map's (reloc_corr_set_map*)
// and the search's (reloc_corr_configure).
struct CorrState {
    int w = 0, h = 0, mp = 0;            // the map: cells, words per packed row
    double ox = 0, oy = 0, res = 0;
    DevBlock map_block;                  // two packed planes of h x mp words: the dilation goes from one to the other
    uint32_t *plane[2] = {};
    uint32_t *map = nullptr;             // the one that holds the dilated map
    int n_side = 0, min_points = 0, half = 0;      // offsets per axis (0: not configured); the window is 2 * half + 1 cells a side
    double z_lo = 0, z_hi = 0, max_range = 0;
    DevBlock cfg_block;                  // the pointers below lie in it, sized for the limits of reloc_spec.h
    uint32_t *list = nullptr;            // the last tick's scan: the non-zero words of the window's bitmap (row << 5 | word, bits)
    int32_t *surface = nullptr;          // n_side x n_side hits of the last tick
    int32_t *table = nullptr;            // n_side cell offsets
    int32_t *record = nullptr;           // the last tick's record
    bool on() const { return w > 0; }
    bool configured() const { return n_side > 0; }
};

// Route clearance of a context (include/reloc_spec.h "ROUTE"; reloc_route.hip); 0 x 0 = no map, the default: a context that never
// sets a route map or a costmap allocates and launches nothing of it.  Two blocks: the map's (reloc_route_set_map*) and the
// costmap's (reloc_route_set_costmap).
struct RouteState {
    int w = 0, h = 0, mp = 0, ws = 0;    // the map: cells, words per packed row, bytes per row of the two byte planes (32 * mp)
    int cap = 0;
    DevBlock block;                      // the pointers below lie in it
    uint32_t *bits = nullptr;            // h x mp: the occupied plane with the stamps, one bit per cell
    uint8_t *rowd = nullptr;             // h x ws: capped distance to the nearest occupied cell of the same row
    uint8_t *clear = nullptr;            // h x ws: the clearance plane (d)
    int32_t *row_remap = nullptr, *col_remap = nullptr;      // h and w entries (e)
    int cw = 0, ch = 0;                  // the costmap: cells
    DevBlock cost;                       // ch x cw int8, a block of its own
    bool on() const { return w > 0; }
    bool has_cost() const { return cw > 0; }
};

// Local obstacle perception of a context (include/reloc_spec.h "OBSTACLE"; reloc_obstacle.hip); nothing configured and no block
// taken is the default: a context that never calls reloc_obs_* allocates and launches nothing of it.  Two blocks: what a frame
// leaves (taken by the first call that reads a depth image) and the grid's (reloc_obs_grid_configure).
struct ObstacleState {
    // the traversability filter (d), reloc_obs_set_filter; bh == 0: off
    int bh = 0, bw = 0, min_count = 0, n_cov = 0;
    float f_lo = 0, f_hi = 0, f_fill = 0;
    double var_thresh = 0, min_solid = 0;
    DevBlock frame_block;                // the pointers below lie in it
    uint8_t *mask = nullptr;             // the last frame's block mask, max_w * max_h / RELOC_OBS_MIN_BLOCK^2 bytes
    float *prof = nullptr;               // RELOC_OBS_MAX_COLS: the last profile ...
    int32_t *cnt = nullptr;              // ... and its counts
    // the grid (e), reloc_obs_grid_configure; cells == 0: none
    int cells = 0, step = 0, q = 0, min_valid = 0, use_filter = 0, cur = 0;
    double res = 0;
    float decay = 0, hit = 0, hit_nb = 0, obstacle_hits = 0, lo = 0, hi = 0;
    DevBlock grid_block;                 // the pointers below lie in it
    float *grid[2] = {};                 // grid[cur] holds the grid, an update writes the other one
    uint8_t *image = nullptr;            // cells x cells: the debug image of the last reloc_obs_grid_read
    int32_t *stats = nullptr;            // 2: cells >= obstacle_hits, the maximum's bits
    double *dirs_host = nullptr;         // pinned, RELOC_OBS_MAX_GRID_COLS pairs: the directions of an enqueue-only update ...
    hipEvent_t dirs_read = nullptr;      // ... and the copy out of it: the next such update waits for it before it overwrites them
    bool filter_on() const { return bh > 0; }
    bool on() const { return cells > 0; }
};

// What the five ORB kernels read and write of one frame, in the form they take it: a launch carries a FrameTable of these in
// its kernel arguments (blockIdx.y = frame).
struct OrbFrame {
    const OrbTable *tab; const PyrTile *tiles; const int32_t *rz; const uint8_t *src;
    uint8_t *pyr, *nms, *blur; int32_t *hist, *cand_cnt; uint32_t *cand_key; float *cand_resp; int32_t *dbg_cut;
    int32_t *kp_cnt; uint32_t *kp_key; float *kp_resp; float *f_xy, *f_size, *f_angle, *f_resp; int32_t *f_oct; uint8_t *f_desc;
    int32_t *f_count;
    const uint8_t *mask;    // mask pyramid of the frame (geometry of pyr), read by the MASKED kernels only
};
static_assert(sizeof(OrbFrame) == 184, "OrbFrame travels in the kernel arguments of the ORB launches (DESIGN.md)");

// ORB front end of a context (reloc_orb.hip): the blocks orb_alloc sized for the context's capacity and the geometry of the
// frame size orb_prepare last published.
struct OrbState {
    int w = 0, h = 0, nfeat = 0;   // the geometry tab, lds and the device tables were built for; w == 0: none
    OrbParams plan_prm;            // ... and the ORB parameters of that plan
    OrbParams prm;                 // the context's persistent ORB parameters (reloc_set_orb_params); a per-call set never lands here
    OrbTable tab = {};             // host copy of the device table buf.tab
    PyrLds lds = {};               // LDS layout of k_pyramid, its workgroups and its dynamic LDS
    int ntiles = 0, lds_bytes = 0;
    OrbCaps caps = {};             // bytes of each of buf.pyr / nms / blur (and of a mask pyramid), entries of buf.rz and buf.tiles
    DevBlock fixed, arenas;        // what buf points into: the arenas (pyr, blur, nms) grow with the ORB parameters, the rest is fixed
    // Device buffers, as the kernels take them; src and mask stay NULL here, a launch sets them in its copy.  tab, tiles, rz:
    // the tables of the geometry above.  pyr, blur, nms: pyramid levels, blurred levels and NMS-kept FAST score maps
    // (stage-1 source, parity tap), one geometry.  hist: NLEV x 256 score histograms.  cand_*: stage-1 lists (NLEV counters,
    // NLEV x STAGE1_CAP keys y << 16 | x and Harris responses).  kp_*: the kept keypoints in raster order per level.  dbg_cut:
    // NLEV stage-1 cut scores of the last frame.  f_*: the frame's features, max_feat rows, and their count.
    OrbFrame buf = {};
    OrbMaskStage mask;             // detection mask between NMS and the stage-1 cut
};

// Tick, match and PnP scratch of a context (allocated and released by reloc_tick.hip); every pointer is device memory
// except res_host / res_ext.
struct TickState {
    DevBlock block;                  // every device pointer below lies in it (tick_alloc)
    int32_t *cand_ids = nullptr;     // MAX_CAND candidate records of the current tick
    int32_t *cand_n = nullptr;       // 1
    int32_t *flags = nullptr;        // [0] relocating: the candidates came from the whole-database search
    int32_t *m_qidx = nullptr, *m_tidx = nullptr, *m_dist = nullptr;    // MAX_CAND x MAX_REC_ROWS match lists of the emit pass
    int32_t *m_n = nullptr;          // MAX_CAND list lengths; behind them MAX_CAND more, written under RELOC_MATCH_RATIO only:
                                     // the lengths PnP reads there, 0 where the record-length gate closed (tick_pnp_lengths)
    float *p_obj = nullptr, *p_img = nullptr;     // MAX_CAND x MAX_REC_ROWS x {3, 2}: the 3-D / 2-D pairs PnP is given
    double *p_Rt = nullptr;          // MAX_CAND x MAX_HYP x 12
    int32_t *p_cnt = nullptr;        // MAX_CAND x MAX_HYP
    int32_t *p_inl = nullptr;        // MAX_CAND x MAX_REC_ROWS
    PnpOut *p_out = nullptr;         // MAX_CAND
    TickResult *res = nullptr;       // 1: the result record on the device
    TickResult *res_host = nullptr;  // the same record in pinned host memory, written by k_tick_finalize
    TickResult *res_ext = nullptr;   // caller's pinned record for the next ticks (reloc_tick_result_to), or NULL
    bool failed = false;             // the last tick entry point on this context returned an error before its result record was
                                     // enqueued: reloc_tick_wait / reloc_tick_result* report RELOC_E_STATE instead of the previous tick's record
    int32_t seq = 0;                 // stamp of the last tick enqueued (TickResult.pad[0] of its host records); 0: none yet
};

struct reloc_ctx {
    int device = 0;
    int max_w = 0, max_h = 0, max_feat = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    int num_cu = 256;

    // profiling
    int prof_on = 0;
    // ring of event pairs per stopwatch: large enough that a measurement of a few hundred launches never has to wait for
    // the device in the middle (prof_flush synchronises)
    struct ProfSlot { hipEvent_t a[RELOC_PROF_RING], b[RELOC_PROF_RING]; int n = 0; float total = 0.f; int launches = 0; bool init = false; } prof[RELOC_PROF_COUNT];

    DevBlock scratch[8];           // generic scratch, grown on demand by the host-pointer entry points (HostStaging)

    OrbState orb;                  // reloc_orb.hip
    DevBlock frame_block;
    uint8_t *frame_img = nullptr;  // staging plane of the host-pointer entry points (image stages, recording, tick, ORB): the
                                   // caller's frame on the device, max_w * max_h * frame_img_bpp bytes; no ORB state
    int frame_img_bpp = 0;         // 3 from creation, 4 once a 4-byte pixel format was enabled or converted (frame_img_reserve)

    CameraModel cam;
    // the image chain's stages in its order (reloc_image.hip); a stage's buffers are one block, taken on its first enable
    struct { BayerStage bayer; PixfmtStage pixfmt; ResizeStage resize; RectifyStage rectify; ClaheStage clahe; } img;

    // ---- matcher parameters (reloc_set_params) and match policy (reloc_set_match_policy) ----
    reloc_params prm;
    MatchPolicy match;
    StereoState stereo;              // reloc_stereo.hip
    OccState occ;                    // reloc_occupancy.hip
    CorrState corr;                  // reloc_correlation.hip
    RouteState route;                // reloc_route.hip
    ObstacleState obs;               // reloc_obstacle.hip
    int scan_gens = 0;               // RELOC_SCAN_GENS (developer switch), read once at creation: n > 0 = single whole-database
                                     // scans in the form of batched ones (n generations of row budgets + sweepers, launch_db_count)
    DevBlock scan_block;
    uint32_t *scan_ticket = nullptr; // SCAN_TICKET_WORDS counters of the whole-database scans (scan_alloc, reloc_scan.hip)

    // ---- database: two arenas; db_sel names the selected one (ctx_db below), reloc_db_select only changes db_sel ----
    DbArena db_slot[2];
    int db_sel = 0;
    DevBlock accum_block;
    AccumResult *accum_res = nullptr;   // 1

    TickState tick;                  // reloc_tick.hip
    int exclusive_hint = -1;         // reloc_set_exclusive: 1 = this ctx is the only stream of work on the GPU, 0 = it is not,
                                     // -1 (default) = it is while it is the only live context of this process (ctx_alone())
    bool local_two_stage = false;    // developer switch RELOC_LOCAL_TWO_STAGE=1: local candidates by k_topk_part + k_candidates_local
};

// The one staging path of the host-pointer entry points, on the context's stream: scratch slots, copies in, launches,
// copies out, finish.  The first error sticks (rc) and turns everything behind it into a no-op, so an entry point reads as
// the straight sequence; finish() synchronises whenever something was enqueued, also behind an error -- no copy from or to
// the caller's memory is in flight when an entry point returns, failed or not.  Slot numbers stay with the entry point: they
// say which calls may overlap.  A download whose size the device decides takes two phases: count(), then the rows.
struct HostStaging {
    reloc_ctx *ctx;
    int rc = RELOC_OK;
    bool pending = false;       // work enqueued since the last synchronisation
    void hip(hipError_t e, const char *what);       // a HIP call's result: the first failure becomes rc and the error text
    void *slot_bytes(int s, int64_t bytes);         // scratch slot s, grown with headroom when too small; NULL after an error
    template <typename T>
    T *slot(int s, int64_t count) { return (T *)slot_bytes(s, count * (int64_t)sizeof(T)); }       // NULL after an error
    void copy(void *dst, const void *src, int64_t bytes, hipMemcpyKind kind)
    {
        run([&] { hip(hipMemcpyAsync(dst, src, (size_t)bytes, kind, ctx->stream), "hipMemcpyAsync"); return rc; });
    }
    void upload(void *dst, const void *src, int64_t bytes) { copy(dst, src, bytes, hipMemcpyHostToDevice); }
    void download(void *dst, const void *src, int64_t bytes) { copy(dst, src, bytes, hipMemcpyDeviceToHost); }
    // count elements of a host array into scratch slot s
    template <typename T>
    T *upload_slot(int s, const T *src, int64_t count) { T *d = slot<T>(s, count); upload(d, src, count * (int64_t)sizeof(T)); return d; }
    // rows of row_bytes, sstride apart at the caller's, dense on the device
    void upload_rows(void *dst, const void *src, int row_bytes, int rows, int sstride)
    {
        run([&] { hip(hipMemcpy2DAsync(dst, row_bytes, src, sstride, row_bytes, rows, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy2DAsync"); return rc; });
    }
    // rows of row_bytes, sstride apart on the device, dense at the caller's
    void download_rows(void *dst, const void *src, int row_bytes, int rows, int sstride)
    {
        run([&] { hip(hipMemcpy2DAsync(dst, row_bytes, src, sstride, row_bytes, rows, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy2DAsync"); return rc; });
    }
    template <typename K, typename... A>
    void launch(K kern, dim3 grid, dim3 block, A... args)
    {
        run([&] { hipLaunchKernelGGL(kern, grid, block, 0, ctx->stream, args...); hip(hipGetLastError(), "kernel launch"); return rc; });
    }
    // anything that enqueues on the stream and returns a RELOC_ code (the library's stage launchers)
    template <typename Fn>
    void run(Fn fn) { if (!rc) { pending = true; rc = fn(); } }
    int finish() { if (pending) hip(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"); pending = false; return rc; }
    // first phase of a two-phase download: the device's count, 0 after an error
    int32_t count(const int32_t *dev) { int32_t n = 0; download(&n, dev, 4); return finish() ? 0 : n; }
};
void reloc_prof_begin(reloc_ctx *ctx, int which);
void reloc_prof_end(reloc_ctx *ctx, int which);

// the selected database of a context
static inline DbArena &ctx_db(reloc_ctx *ctx) { return ctx->db_slot[ctx->db_sel]; }
static inline const DbArena &ctx_db(const reloc_ctx *ctx) { return ctx->db_slot[ctx->db_sel]; }
// The one way out of a slot: lets go of this holder's reference to the six shared arrays (the last holder frees them),
// frees the arena's own counts / topk_part and leaves the arena value-initialised (reloc_db.hip)
void db_arena_release(DbArena &a);
extern int g_reloc_live_contexts;           // contexts created and not yet destroyed in this process (reloc_ctx.hip)
static inline bool ctx_alone(const reloc_ctx *c)
{
    return c->exclusive_hint > 0 || (c->exclusive_hint < 0 && __atomic_load_n(&g_reloc_live_contexts, __ATOMIC_RELAXED) == 1);
}

// Stage launchers shared between translation units.  Each takes the n <= RELOC_BATCH_MAX contexts of one call (one stream,
// equal geometry, parameters and database: ctx_batch_check in reloc_tick.hip) and makes ONE launch per kernel of its stage.
// The ORB, PnP and tick kernels take a FrameTable of per-frame structs by value and index it with the last grid dimension;
// everything that differs between frames (buffers, seed, base pose, sequence stamp, masks) is a field of that struct, the
// other kernel arguments are what the frames share.  Each kernel exists for N = 1 (one frame, a 1-slot table) and for
// N = RELOC_BATCH_MAX (2..8 frames); a launcher is written once as a template on N and picked by n == 1.  Two kernels keep
// a pointer-argument form for one frame beside the 8-slot table form, each for a measured reason stated at the kernel:
// k_pyramid (reloc_orb.hip) and k_topk_counts (reloc_tick.hip).  (The scan family keeps its own single / batch kernels:
// reloc_hamming.h.)
// latency: kernels sized for latency instead of for fitting beside another stream's whole-database scan (512-thread
// pyramid, 8-wave emit pass, unconstrained k_pnp_finish); only a single frame (N == 1) ever gets them.
constexpr int RELOC_BATCH_MAX = 8;          // frames per batched launch (reloc_tick_batch_dev, reloc_shard_*_batch_dev)

// N is 1 or RELOC_BATCH_MAX.  The 1-slot table never reads the block index.
template <typename Frame, int N> struct FrameTable {
    Frame f[N];
    __device__ __forceinline__ const Frame &at(unsigned i) const { return f[N == 1 ? 0 : i]; }
};

// Visits the RELOC_BATCH_MAX slots of a frame table: fn(slot, ctx, frame) with frame = slot for the n frames of the call and
// frame 0 for the padding slots (never read: the grid holds n frames).  A one-frame launch takes slot 0 of it.
template <typename Fn>
static inline void frame_slots(reloc_ctx *const *ctxs, int n, Fn fn)
{
    for (int f = 0; f < RELOC_BATCH_MAX; ++f) fn(f, ctxs[f < n ? f : 0], f < n ? f : 0);
}
// the table a launch<N> passes: the first N slots of the filled one
template <int N, typename Frame>
static inline FrameTable<Frame, N> frame_table(const FrameTable<Frame, RELOC_BATCH_MAX> &b)
{
    FrameTable<Frame, N> t;
    for (int f = 0; f < N; ++f) t.f[f] = b.f[f];
    return t;
}

// The whole-database scans count the mutual matches of the current descriptors (cur, n_cur_max capacity, count on the
// device at n_cur_dev when non-NULL) with every record of the context's database into counts[record]: one frame
// (launch_db_count) or one per context of a batch (launch_db_scan_batch).
int launch_db_count(reloc_ctx *ctx, const uint8_t *cur, const int32_t *n_cur_dev, int n_cur_max, int32_t *counts,
                    const ScanMask &mask = {});
int launch_db_scan_batch(reloc_ctx *const *ctxs, int n, const double *q, double cos_tol, bool auto_mode, bool heading_mask = true);
// The same scans under RELOC_MATCH_RATIO: counts[record] = Lowe survivors of every context's features against the record
// (k_db_ratio), 0 for records of fewer than min_matches rows.  base_poses: n x 7 (heading mask) or NULL.
int launch_db_ratio_scan(reloc_ctx *const *ctxs, int n, const double *base_poses, double cos_tol, bool auto_mode);
// the emit pass of a tick: match lists, with their 3-D / 2-D pairs, of every context's candidate records (reloc_scan.hip)
int launch_tick_emit(reloc_ctx *const *ctxs, int n, bool latency);
// the list lengths of a context's candidates as PnP takes them (see TickState::m_n)
static inline const int32_t *tick_pnp_lengths(const reloc_ctx *c) { return c->tick.m_n + (c->match.ratio_on() ? MAX_CAND : 0); }
// re-derives the headings of both slots' records from the camera mounting; grows the selected arena (reloc_db.hip)
int db_reindex(reloc_ctx *ctx);
int db_reserve(reloc_ctx *ctx, int64_t cap_records, int64_t cap_rows);
inline bool db_ready(const reloc_ctx *ctx)
{
    const DbArena &db = ctx_db(ctx);
    return db.desc && db.off && db.pose && db.xy_heading && db.counts && db.records > 0;
}
// the fixed blocks of a new context, each stage's by its own file: ORB (reloc_orb.hip), scan counters (reloc_scan.hip), tick /
// match / PnP scratch with the pinned result record (reloc_tick.hip; tick_release lets go of that record), the staging plane
// of bpp bytes per pixel (reloc_image.hip; grows once, to 4)
int frame_img_reserve(reloc_ctx *ctx, int bpp);
int orb_alloc(reloc_ctx *ctx);
int scan_alloc(reloc_ctx *ctx);
int tick_alloc(reloc_ctx *ctx);
void tick_release(reloc_ctx *ctx);
// tables and tiles of a frame size on the device (cached: one geometry per context); a failure leaves no geometry
int orb_prepare(reloc_ctx *ctx, int w, int h, int nfeatures, const OrbParams &prm);
// ORB of frame f = srcs[f] into ctxs[f]'s feature buffers; chain -> the frames of the image chain, of
// image_chain_frame_bpp bytes per pixel: interleaved 3-channel frames (gray fused), raw mosaics with the Bayer stage on, or
// frames of the contexts' pixel format (a mono8 frame is one channel and still a frame of the chain); the
// chain first when the contexts have stages on; with the downscale stage on, w x h is the source size and the features are
// those of the working frame.  !chain -> a caller's gray planes, never through the chain.  The chain's frames are detected
// under the contexts' persistent mask; call_mask: under the mask whose level 0 the caller left in mask.call (reloc_orb.hip).
// Every frame runs with its context's persistent ORB parameters, which a batch must agree on; call_prm: one frame with
// these instead, the blocks already grown for them (orb_grow).
int orb_run(reloc_ctx *const *ctxs, int n, const uint8_t *const *srcs, int w, int h, int stride, bool chain, int order,
            int nfeatures, bool latency, bool call_mask = false, const OrbParams *call_prm = nullptr);
// The image chain of a context's stages (reloc_image.hip states their order).  chain: the frames are frames of the chain
// (orb_run).  The checks stand before orb_prepare (the Bayer stage, the pixel format and the downscale stage; w x h becomes
// the working frame) and behind that of context f (rectification, CLAHE); _gray runs the stages on the frames and leaves
// *srcs / *stride / *channels describing the last plane written, or the frame itself; _depth takes a
// depth image through resize and rectification (nearest), *w x *h becomes the working frame; _frame_bpp: bytes per pixel of
// the frames that the entry points take (3; 1 for raw mosaics and mono8; 2 for 4:2:2; 4 for BGRA / RGBA).
int image_chain_frame_bpp(const reloc_ctx *c);
int image_chain_check(reloc_ctx *const *ctxs, int n, bool chain, int *w, int *h);
int image_chain_check_prepared(reloc_ctx *const *ctxs, int f, int n, bool chain, int w, int h);
int image_chain_gray(reloc_ctx *const *ctxs, int n, bool chain, const uint8_t *const **srcs, int sw, int sh, int w, int h,
                     int *stride, int *channels, int flags, const uint8_t **planes);
int image_chain_depth(reloc_ctx *ctx, const uint16_t *depth_dev, int *w, int *h, const uint16_t **out);
// plain gray conversion of a 3-channel frame on c's stream into dense rows of w bytes (reloc_image.hip, k_gray_plain)
int image_gray_plain(reloc_ctx *c, const uint8_t *src, int w, int h, int sstride, int order, uint8_t *dst);
// Sparse stereo depth (reloc_stereo.hip).  stereo_frame: the right eye's frame (device memory, a frame of right's chain, w x h
// as handed in) through right's chain on right's stream, then k_stereo_depth for the keypoints of ctx's last ORB frame on
// ctx's stream into ctx->stereo.mm / disp / status; the streams are ordered by events in both directions.  *ww x *wh: the
// working frame.  stereo_release: the events of a context that had stereo on.
int stereo_frame(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *img_right_dev, int w, int h, int order, int *ww, int *wh);
void stereo_release(reloc_ctx *ctx);
// What the sparse and the dense pass (reloc_stereo_dense.hip) share of reloc_stereo.hip.
// A semi-global setting as a pass takes it: the directions (bit b of mask selects direction b) and the two penalties.
struct StereoSgm { int mask, p1, p2; };
// What a stateless stereo call checks after its pointers, in this order: fx finite and positive, the matcher's parameters, the
// semi-global setting (sgm == NULL: a plain pass), the frame within ctx's capacity.
int stereo_call_check(const reloc_ctx *ctx, int w, int h, double fx, double baseline_m, int min_disparity, int num_disparities,
                      int uniqueness, int lr_check, int cost, const StereoSgm *sgm);
// What a stereo pass checks of its pair of contexts before it enqueues anything: what an entry point checks (stereo_pair_entry),
// then two contexts of one device and one gray conversion, the two chains in agreement as in a batch; *ww x *wh: the working frame.
int stereo_pair_check(reloc_ctx *ctx, reloc_ctx *right, int w, int h, int *ww, int *wh);
// The gray planes of a pass, plane[e] with rows of stride[e] bytes, e = 1 the right eye: the right eye's chain on right's stream,
// the left eye's (lsrc == NULL: none, plane[0] is not written) on ctx's.  The streams are ordered by events in both directions:
// right's goes on behind what ctx's holds so far -- the copy that brought the right frame (a _dev caller orders its frames on
// ctx's stream) and the last stereo kernel, which still reads the right chain's planes -- and ctx's behind the right eye's chain.
int stereo_gray_planes(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *lsrc, const uint8_t *rsrc, int w, int h, int ww, int wh,
                       int order, const uint8_t *plane[2], int stride[2]);
// The census planes of a pass's eyes (reloc_census.hip; "STEREO, census").  stereo_census_alloc: the context's census block on
// its first census pass, before the pass's stopwatch bracket.  stereo_census_launch: k_census over both eyes (device pointers,
// w x h, each with its own stride) on ctx's stream; afterwards the pointers name ctx's census planes and both strides are w.
int stereo_census_alloc(reloc_ctx *ctx);
void stereo_census_launch(reloc_ctx *ctx, const uint8_t *&left, int &lstride, const uint8_t *&right, int &rstride, int w, int h);
// the pinned direction table and its event of a context that updated its obstacle grid from the stereo plane (reloc_obstacle.hip)
void obs_release(reloc_ctx *ctx);
// blocks of a 1-D grid-stride launch of 256 threads over n elements: at least one, at most max_blocks
static inline unsigned grid_1d(int64_t n, int max_blocks) { const int64_t b = (n + 255) / 256; return (unsigned)(b < 1 ? 1 : b < max_blocks ? b : max_blocks); }
// an entry point that needs a map the context lacks: RELOC_E_STATE
static inline int need_map(bool on, const char *who, const char *what, const char *setter)
{
    if (!on) reloc_set_error("%s: no %s map on this context (%s)", who, what, setter);
    return on ? RELOC_OK : RELOC_E_STATE;
}
// an occupied plane on the device (h x w uint8, non-zero = occupied; from_units: the occupancy map's int8 units, occupied from
// RELOC_OCC_UNITS_OCC) as h packed rows of mp = ceil(w / 32) words, the bits beyond column w - 1 clear (reloc_correlation.hip)
void corr_pack_plane(HostStaging &st, const void *plane, bool from_units, uint32_t *bits, int w, int h, int mp);
// Dense stereo depth (reloc_stereo_dense.hip): both eyes' frames (ctx->frame_img, right->frame_img, w x h as handed in)
// through the gray half of their chains, each on its own stream, no ORB; then k_stereo_dense and k_stereo_dense_finish on ctx's stream into ctx->stereo.dense
// (mm: dense rows of *ww uint16); with reloc_set_stereo_sgm on, the semi-global pass in their place, into the same planes.
// Checks stereo on, right != ctx, capacity and the chains' agreement.
int stereo_dense_frame(reloc_ctx *ctx, reloc_ctx *right, int w, int h, int order, int *ww, int *wh);
// the speckle stage on the w x h planes of ctx's dense pass with ctx's speckle setting (window > 0), on ctx's stream
// (reloc_speckle.hip)
int stereo_speckle_launch(reloc_ctx *ctx, int w, int h);
// PnP-RANSAC of every context's candidates with the matcher parameters of ctxs[0]; seeds: one per frame, or NULL (reloc_pnp.hip)
int pnp_run_candidates(reloc_ctx *const *ctxs, int n, const uint64_t *seeds, bool latency);
