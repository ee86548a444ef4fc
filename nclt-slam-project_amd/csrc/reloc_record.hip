// reloc_record.hip -- teach-side record builder on gfx950.
//
// Serves VisualLandmarkRecorder._tick after ORB (reference R:247-288): keypoint rounding, border and
// ground masks, depth lookup (mm -> m), 3x3 non-zero depth standard deviation, range / variance gates,
// pin-hole back-projection.  The reference does this in NumPy with a Python loop per keypoint
// (R:262-266); NumPy's arithmetic is the specification here, so every expression below mirrors the
// NumPy dtype rules of the reference's lines:
//   np.round(float32)            -> round half to even in float32
//   depth.astype(float32)/1000.0 -> float32 division
//   patch[patch > 0.01].std()    -> float32 pairwise sum (numpy's 8-accumulator tree for n >= 8,
//                                   running sum from 0 for n < 8), mean, squared deviations, mean, sqrt
//   (uu - CX) * d_c / FX         -> int32 - python float = float64, * float32 = float64, / float64,
//                                   stacked with float32 z and cast to float32
// One lane per keypoint; survivors are compacted in keypoint order by a block-wide scan.
// Lens distortion (include/reloc_spec.h): k_record<true> / k_accumulate<true> back-project through the inverse model,
//   (x_u, y_u) = undistort(u, v); X = x_u * z, Y = y_u * z in float64, cast to float32,
// with the same pixel-based gates (the kept rows do not change).
// Depth source: KPD.  false: the depth image.  true: a per-keypoint uint16 array indexed by the keypoint's row in the frame's ORB
// output, the millimetres of k_stereo_depth (reloc_stereo.hip; include/reloc_spec.h "STEREO"): dz = (float)kp_mm[i] / 1000.0f,
// k_record skips the 3x3 patch and takes sd = 0, everything else is the same expression -- border, ground, range,
// back-projection, compaction, pose and index of an accumulated record.
// DIST and KPD are template parameters of the two __global__ kernels, so each of the eight instantiations holds only its own
// branch.  What the two kernels have in common -- the keypoint's pixel, its depth, the back-projection, the descriptor copy and
// the compaction (block_rank, reloc_teach.h) -- are __forceinline__ functions templated the same way; the compiler schedules
// their bodies with the caller's, so an instantiation's instructions are not those of a hand-inlined copy, only its results are
// (DESIGN.md "Teach-side kernels" has the registers and instruction counts before and after the functions were shared).
#include "reloc_teach.h"

// keypoint i of the frame's ORB output, its rounded pixel and (keypoint_depth) its depth in metres
struct KeyPixel { float x, y, dz; int u, v; };

// reads and rounds the keypoint; true iff the pixel has all eight neighbours in the w x h frame
__device__ __forceinline__ bool keypoint_pixel(const float *__restrict__ f_xy, int i, int w, int h, KeyPixel &k)
{
    k.x = f_xy[2 * i]; k.y = f_xy[2 * i + 1];
    k.u = (int)rintf(k.x); k.v = (int)rintf(k.y);
    return k.u >= 1 && k.u < w - 1 && k.v >= 1 && k.v < h - 1;
}

// KPD: depth holds the millimetres per keypoint, else the depth image with rows of dstride pixels
template <bool KPD>
__device__ __forceinline__ float keypoint_depth(const uint16_t *__restrict__ depth, int dstride, int i, int u, int v)
{
    return __fdiv_rn((float)(KPD ? depth[i] : depth[(size_t)v * dstride + u]), 1000.0f);
}

// camera-frame point of the rounded pixel (u, v) at depth dz: pinhole, or through the inverse distortion model
template <bool DIST>
__device__ __forceinline__ void back_project(double fx, double fy, double cx, double cy, const DistCoef &dc, int u, int v, float dz,
                                             float *o)
{
    if constexpr (DIST) {
        const double K4[4] = {fx, fy, cx, cy};
        double xu, yu;
        undistort_norm(dc, K4, (double)u, (double)v, xu, yu);
        o[0] = (float)__dmul_rn(xu, (double)dz);
        o[1] = (float)__dmul_rn(yu, (double)dz);
    } else {
        o[0] = (float)__ddiv_rn(__dmul_rn(__dsub_rn((double)u, cx), (double)dz), fx);
        o[1] = (float)__ddiv_rn(__dmul_rn(__dsub_rn((double)v, cy), (double)dz), fy);
    }
    o[2] = dz;
}

// row pos of a record from keypoint i: position, camera-frame point, descriptor
template <bool DIST>
__device__ __forceinline__ void keypoint_row(const KeyPixel &k, int i, int pos, double fx, double fy, double cx, double cy,
                                             const DistCoef &dc, const uint8_t *__restrict__ f_desc, float *__restrict__ o_xy,
                                             float *__restrict__ o_pts, uint8_t *__restrict__ o_desc)
{
    o_xy[2 * pos] = k.x; o_xy[2 * pos + 1] = k.y;
    back_project<DIST>(fx, fy, cx, cy, dc, k.u, k.v, k.dz, o_pts + 3 * pos);
    const uint4 *s = reinterpret_cast<const uint4 *>(f_desc + (size_t)i * 32);
    uint4 *d = reinterpret_cast<uint4 *>(o_desc + (size_t)pos * 32);
    d[0] = s[0]; d[1] = s[1];
}

struct RecordParams {
    double fx, fy, cx, cy;
    float depth_min, depth_max, var_max;
    int ground_y;
    int w, h;
};

// float32 sum with numpy's pairwise order for n <= 9
__device__ float np_sum9(const float *a, int n)
{
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r = __fadd_rn(r, a[i]);
        return r;
    }
    float r = __fadd_rn(__fadd_rn(__fadd_rn(a[0], a[1]), __fadd_rn(a[2], a[3])),
                        __fadd_rn(__fadd_rn(a[4], a[5]), __fadd_rn(a[6], a[7])));
    for (int i = 8; i < n; ++i) r = __fadd_rn(r, a[i]);
    return r;
}

template <bool DIST, bool KPD = false>
__global__ __launch_bounds__(1024) void k_record(const float *__restrict__ f_xy, const uint8_t *__restrict__ f_desc,
                                                 const int32_t *__restrict__ f_count, int max_feat,
                                                 const uint16_t *__restrict__ depth, int dstride, RecordParams p,
                                                 float *__restrict__ o_xy, uint8_t *__restrict__ o_desc,
                                                 float *__restrict__ o_pts, int32_t *__restrict__ o_idx,
                                                 int32_t *__restrict__ o_n, DistCoef dc)
{
    RELOC_SMALL_KERNEL_PRIO();
    __shared__ int s_wsum[16];
    const int tid = threadIdx.x;
    const int n = min(*f_count, max_feat);
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        bool keep = false;
        KeyPixel k = {};
        if (i < n && keypoint_pixel(f_xy, i, p.w, p.h, k) && k.v > p.ground_y) {
            const int u = k.u, v = k.v;
            k.dz = keypoint_depth<KPD>(depth, dstride, i, u, v);
            float sd = 0.0f;                                       // KPD: no patch
            if constexpr (!KPD) {
                float vals[9];
                int cnt = 0;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const float m = __fdiv_rn((float)depth[(size_t)(v + dy) * dstride + (u + dx)], 1000.0f);
                        if (m > 0.01f) vals[cnt++] = m;
                    }
                sd = 999.0f;
                if (cnt >= 3) {
                    const float mean = __fdiv_rn(np_sum9(vals, cnt), (float)cnt);
                    float sq[9];
                    for (int j = 0; j < cnt; ++j) { const float d = __fsub_rn(vals[j], mean); sq[j] = __fmul_rn(d, d); }
                    sd = __fsqrt_rn(__fdiv_rn(np_sum9(sq, cnt), (float)cnt));
                }
            }
            keep = k.dz > p.depth_min && k.dz < p.depth_max && sd < p.var_max;
        }
        int total;
        const int pos = block_rank(keep, s_wsum, base, total);
        if (keep) {
            keypoint_row<DIST>(k, i, pos, p.fx, p.fy, p.cx, p.cy, dc, f_desc, o_xy, o_pts, o_desc);
            o_idx[pos] = i;
        }
        base += total;
    }
    if (tid == 0) *o_n = base;
}

// the recorder's gates on the w x h working frame of ctx's camera
static RecordParams record_params(const reloc_ctx *ctx, int w, int h)
{
    RecordParams p;
    p.fx = ctx->cam.K4[0]; p.fy = ctx->cam.K4[1]; p.cx = ctx->cam.K4[2]; p.cy = ctx->cam.K4[3];
    p.depth_min = RELOC_DEPTH_MIN_M; p.depth_max = RELOC_DEPTH_MAX_M; p.var_max = RELOC_DEPTH_VAR_MAX_M;
    p.ground_y = RELOC_GROUND_Y_THRESHOLD; p.w = w; p.h = h;
    return p;
}

// The rows of one recording on the device (scratch slot 6 of the context), the gates' launch on the frame's ORB output and the
// rows' way to the caller: what reloc_record_frame and reloc_record_frame_stereo share behind their depth source.
struct RecordRows {
    uint8_t *desc = nullptr;
    float *xy = nullptr, *pts = nullptr;
    int32_t *idx = nullptr, *n = nullptr;
    bool alloc(HostStaging &st)
    {
        const int64_t mf = st.ctx->max_feat;
        desc = st.slot<uint8_t>(6, mf * (8 + 32 + 12 + 4) + 64);
        if (st.rc) return false;
        xy = (float *)(desc + mf * 32); pts = xy + mf * 2;
        idx = (int32_t *)(pts + mf * 3); n = idx + mf;
        return true;
    }
    // KPD: depth holds the millimetres per keypoint (dstride unused), else the depth image of the w x h working frame
    template <bool KPD>
    void launch(HostStaging &st, const uint16_t *depth, int w, int h)
    {
        reloc_ctx *ctx = st.ctx;
        const RecordParams p = record_params(ctx, w, h);
        const double *lens = ctx->cam.lens();
        st.launch(lens ? k_record<true, KPD> : k_record<false, KPD>, dim3(1), dim3(1024), ctx->orb.buf.f_xy, ctx->orb.buf.f_desc,
                  ctx->orb.buf.f_count, ctx->max_feat, depth, w, p, xy, desc, pts, idx, n, make_dist(lens));
    }
    // the rows written (0 after an error) into the caller's arrays, each of which may be NULL; *nk = the frame's ORB keypoints
    int32_t download(HostStaging &st, float *h_xy, uint8_t *h_desc, float *h_pts, int32_t *h_idx, int32_t *nk)
    {
        st.download(nk, st.ctx->orb.buf.f_count, 4);
        const int32_t rows = st.count(n);
        if (rows > 0) {
            if (h_xy) st.download(h_xy, xy, (int64_t)rows * 8);
            if (h_desc) st.download(h_desc, desc, (int64_t)rows * 32);
            if (h_pts) st.download(h_pts, pts, (int64_t)rows * 12);
            if (h_idx) st.download(h_idx, idx, (int64_t)rows * 4);
        }
        return rows;
    }
};

// Host-pointer entry point: ORB on the frame, then the gates.  Outputs hold up to the ctx's max_feat
// rows: xy (n,2) f32 keypoints_2d, desc (n,32) u8, pts3d (n,3) f32 keypoints_3d_cam, kp_index (n) i32
// (row of the surviving keypoint in the frame's ORB output); *n_out rows written, *n_kp = ORB keypoints.
RELOC_API int reloc_record_frame(reloc_ctx *ctx, const uint8_t *img, const uint16_t *depth_mm, int w, int h, int order,
                                 int nfeatures, float *xy, uint8_t *desc, float *pts3d, int32_t *kp_index, int32_t *n_out,
                                 int32_t *n_kp)
{
    ARG_CHECK_CTX(ctx, img && depth_mm && n_out && w >= 64 && h >= 64 && nfeatures > 0, "reloc_record_frame");
    if (w > ctx->max_w || h > ctx->max_h) { reloc_set_error("frame exceeds ctx capacity"); return RELOC_E_CAPACITY; }
    *n_out = 0;
    if (n_kp) *n_kp = 0;
    HostStaging st{ctx};
    RecordRows rows;
    if (!rows.alloc(st)) return st.rc;
    const int bpp = image_chain_frame_bpp(ctx);
    st.upload(ctx->frame_img, img, (int64_t)w * h * bpp);
    const uint16_t *depth = st.upload_slot(5, depth_mm, (int64_t)w * h);
    st.run([&] {
        const uint8_t *src = ctx->frame_img;
        if (int rc = orb_run(&ctx, 1, &src, w, h, w * bpp, true, order, nfeatures, true)) return rc;
        return image_chain_depth(ctx, depth, &w, &h, &depth);      // from here on the working frame
    });
    rows.launch<false>(st, depth, w, h);
    int32_t nk = 0;
    const int32_t n = rows.download(st, xy, desc, pts3d, kp_index, &nk);
    if (int rc = st.finish()) return rc;
    *n_out = n;
    if (n_kp) *n_kp = nk;
    return RELOC_OK;
}

// The same with the right eye's frame in the depth image's place (include/reloc_spec.h "STEREO"): ORB on the left frame, the
// right frame through its own context's chain, k_stereo_depth at the keypoints, then the gates on the per-keypoint depth.
RELOC_API int reloc_record_frame_stereo(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *img, const uint8_t *img_right, int w, int h,
                                        int order, int nfeatures, float *xy, uint8_t *desc, float *pts3d, int32_t *kp_index,
                                        int32_t *n_out, int32_t *n_kp, int32_t *n_stereo)
{
    ARG_CHECK_CTX(ctx, right && img && img_right && n_out && w >= 64 && h >= 64 && nfeatures > 0, "reloc_record_frame_stereo");
    if (int rc = stereo_pair_entry(ctx, right, w, h)) return rc;
    *n_out = 0;
    if (n_kp) *n_kp = 0;
    if (n_stereo) *n_stereo = 0;
    StereoPairStaging st(ctx, right);
    RecordRows rows;
    if (!rows.alloc(st)) return st.rc;
    st.upload_pair(img, img_right, w, h);
    st.run([&] {
        const uint8_t *src = ctx->frame_img;
        if (int rc = orb_run(&ctx, 1, &src, w, h, w * image_chain_frame_bpp(ctx), true, order, nfeatures, true)) return rc;
        return stereo_frame(ctx, right, right->frame_img, w, h, order, &w, &h);      // from here on the working frame
    });
    rows.launch<true>(st, ctx->stereo.mm, w, h);
    int32_t nk = 0;
    const int32_t n = rows.download(st, xy, desc, pts3d, kp_index, &nk);
    const int32_t ns = nk < ctx->max_feat ? nk : ctx->max_feat;
    std::vector<uint8_t> status((size_t)(n_stereo && ns > 0 ? ns : 0));
    if (!status.empty()) st.download(status.data(), ctx->stereo.status, ns);
    if (int rc = st.finish()) return rc;
    *n_out = n;
    if (n_kp) *n_kp = nk;
    for (uint8_t s : status) *n_stereo += s == RELOC_STEREO_OK;
    return RELOC_OK;
}

// ---------------------------------------------------------------------------------------------------
// Accumulation (reference M:435-500): after a tick that published nothing, the current frame becomes a new record when
// the matcher has been silent long enough (host-side fact, silence_ok), no filed record lies within min_dist of the
// robot and enough keypoints carry a usable depth.  The record is written straight behind the arena's last row; the
// host adopts it (record / row counts) when it reads AccumResult.  NumPy dtype rules of the reference lines, as above:
//   np.round(pts[:, 0]).astype(int32); (uu >= 1) & (uu < W - 1) & (vv >= 1) & (vv < H - 1)            M:449-453
//   d_c = depth[vv, uu].astype(float32) / 1000.0; ok = (d_c > 0.5) & (d_c < 15.0)                     M:460-461
//   (uu - cx) * d_c / fx in float64, stacked with z and cast to float32                                M:469-473
//   camera pose = base pose (+) static mount, quaternion by scipy's Rotation.from_matrix().as_quat()   M:475-480
struct AccumParams {
    double fx, fy, cx, cy;
    double base_pose[7], b2c_t[3], b2c_R[9];
    double min_dist;
    float zmin, zmax;
    int w, h, min_kpts, silence_ok;
    int64_t L, T;            // records / rows of the database before the append
};

// scipy.spatial.transform.Rotation.from_matrix (Markley's method) followed by as_quat(): x y z w, not canonicalised
__device__ void rot_to_quat_scipy(const double R[9], double q[4])
{
    const double d0 = R[0], d1 = R[4], d2 = R[8], tr = R[0] + R[4] + R[8];
    int choice = 0;
    double best = d0;
    if (d1 > best) { best = d1; choice = 1; }
    if (d2 > best) { best = d2; choice = 2; }
    if (tr > best) { best = tr; choice = 3; }
    if (choice != 3) {
        const int i = choice, j = (i + 1) % 3, k = (j + 1) % 3;
        q[i] = 1 - tr + 2 * R[3 * i + i];
        q[j] = R[3 * j + i] + R[3 * i + j];
        q[k] = R[3 * k + i] + R[3 * i + k];
        q[3] = R[3 * k + j] - R[3 * j + k];
    } else {
        q[0] = R[7] - R[5];
        q[1] = R[2] - R[6];
        q[2] = R[3] - R[1];
        q[3] = 1 + tr;
    }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int c = 0; c < 4; ++c) q[c] = q[c] / n;
}

template <bool DIST, bool KPD = false>
__global__ __launch_bounds__(1024) void k_accumulate(const float *__restrict__ f_xy, const uint8_t *__restrict__ f_desc,
                                                     const int32_t *__restrict__ f_count, int max_feat,
                                                     const uint16_t *__restrict__ depth, int dstride, AccumParams p,
                                                     const TickResult *__restrict__ tick, double *__restrict__ xyh,
                                                     uint8_t *__restrict__ db_desc, float *__restrict__ db_pts3d,
                                                     float *__restrict__ db_kp2d, int64_t *__restrict__ db_off,
                                                     double *__restrict__ db_pose, AccumResult *__restrict__ res,
                                                     DistCoef dc)
{
    RELOC_SMALL_KERNEL_PRIO();
    __shared__ int s_wsum[16];
    __shared__ double s_wmin[16];
    __shared__ double s_near;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int oc = tick->outcome;
    const bool wanted = p.silence_ok && (oc == RELOC_OUT_NO_CANDIDATES || oc == RELOC_OUT_NO_PNP_ACCEPT || oc == RELOC_OUT_CONSISTENCY_FAIL);
    if (!wanted) {                                               // block-uniform
        if (tid == 0) { res->appended = 0; res->n_kpts = 0; res->nearest_m = -1.0; }
        return;
    }
    // nearest filed record (M:444-446)
    double dmin = 1e300;
    for (int64_t i = tid; i < p.L; i += 1024) {
        const double dx = xyh[4 * i] - p.base_pose[0], dy = xyh[4 * i + 1] - p.base_pose[1];
        dmin = fmin(dmin, sqrt(dx * dx + dy * dy));
    }
    for (int d = 32; d >= 1; d >>= 1) dmin = fmin(dmin, __shfl_xor(dmin, d));
    if (lane == 0) s_wmin[wave] = dmin;
    __syncthreads();
    if (tid == 0) {
        double m = s_wmin[0];
        for (int w = 1; w < 16; ++w) m = fmin(m, s_wmin[w]);
        s_near = m;
    }
    __syncthreads();
    const double nearest = s_near;
    if (nearest < p.min_dist) {
        if (tid == 0) { res->appended = 0; res->n_kpts = 0; res->nearest_m = nearest; }
        return;
    }
    const int n = min(*f_count, max_feat);
    uint8_t *o_desc = db_desc + p.T * 32;
    float *o_pts = db_pts3d + p.T * 3, *o_xy = db_kp2d + p.T * 2;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        bool keep = false;
        KeyPixel k = {};
        if (i < n && keypoint_pixel(f_xy, i, p.w, p.h, k)) {
            k.dz = keypoint_depth<KPD>(depth, dstride, i, k.u, k.v);
            keep = k.dz > p.zmin && k.dz < p.zmax;
        }
        int total;
        const int pos = block_rank(keep, s_wsum, base, total);
        if (keep) keypoint_row<DIST>(k, i, pos, p.fx, p.fy, p.cx, p.cy, dc, f_desc, o_xy, o_pts, o_desc);
        base += total;
    }
    if (tid == 0) {
        const int cnt = base;
        res->n_kpts = cnt;
        res->nearest_m = nearest;
        if (cnt < p.min_kpts) { res->appended = 0; return; }
        // camera pose from the base pose through the static mount (M:475-480)
        double Rwb[9], Rwc[9], q[4];
        quat_to_rot(p.base_pose[3], p.base_pose[4], p.base_pose[5], p.base_pose[6], Rwb);
        double *pose = db_pose + 7 * p.L;
        for (int r = 0; r < 3; ++r)
            pose[r] = p.base_pose[r] + ((Rwb[3 * r] * p.b2c_t[0] + Rwb[3 * r + 1] * p.b2c_t[1]) + Rwb[3 * r + 2] * p.b2c_t[2]);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                Rwc[3 * r + c] = (Rwb[3 * r] * p.b2c_R[c] + Rwb[3 * r + 1] * p.b2c_R[3 + c]) + Rwb[3 * r + 2] * p.b2c_R[6 + c];
        rot_to_quat_scipy(Rwc, q);
        for (int c = 0; c < 4; ++c) pose[3 + c] = q[c];
        // filed under the VIO position (M:491); heading as for every record (M:233-245, k_db_index)
        double Rq[9];
        quat_to_rot(q[0], q[1], q[2], q[3], Rq);
        const double fx = Rq[0] * p.b2c_R[0] + Rq[1] * p.b2c_R[1] + Rq[2] * p.b2c_R[2];
        const double fy = Rq[3] * p.b2c_R[0] + Rq[4] * p.b2c_R[1] + Rq[5] * p.b2c_R[2];
        const double fn = sqrt(fx * fx + fy * fy);
        xyh[4 * p.L] = p.base_pose[0];
        xyh[4 * p.L + 1] = p.base_pose[1];
        xyh[4 * p.L + 2] = fn > 0 ? fx / fn : 1.0;
        xyh[4 * p.L + 3] = fn > 0 ? fy / fn : 0.0;
        db_off[p.L + 1] = p.T + cnt;
        res->appended = 1;
    }
}

// room for one more record of max_feat rows in the selected database, which must be this context's own
static int accum_reserve(reloc_ctx *ctx)
{
    if (!db_ready(ctx)) { reloc_set_error("no database uploaded"); return RELOC_E_STATE; }
    const DbArena &db = ctx_db(ctx);
    if (db.shared) { reloc_set_error("the selected database is shared from another context (read-only here)"); return RELOC_E_STATE; }
    if (db.records + 1 > db.cap_records || db.rows + ctx->max_feat > db.cap_rows) {
        // grow first (drains the stream): the kernel writes behind the last row without asking
        int rc = db_reserve(ctx, db.cap_records + db.cap_records / 2 + 64, db.cap_rows + db.cap_rows / 2 + 64 * (int64_t)ctx->max_feat);
        if (rc) return rc;
    }
    return RELOC_OK;
}

// k_accumulate on the w x h working frame; KPD: depth = per-keypoint millimetres (reloc_tick_accumulate_stereo_dev)
template <bool KPD>
static int accum_launch(reloc_ctx *ctx, const uint16_t *depth_mm_dev, int w, int h, const double base_pose[7], int silence_ok)
{
    const DbArena &db = ctx_db(ctx);
    AccumParams p;
    const CameraModel &cam = ctx->cam;
    p.fx = cam.K4[0]; p.fy = cam.K4[1]; p.cx = cam.K4[2]; p.cy = cam.K4[3];
    for (int k = 0; k < 7; ++k) p.base_pose[k] = base_pose[k];
    for (int k = 0; k < 3; ++k) p.b2c_t[k] = cam.b2c_t[k];
    for (int k = 0; k < 9; ++k) p.b2c_R[k] = cam.b2c_R[k];
    p.min_dist = ctx->prm.accum_min_dist_m;
    p.zmin = (float)ctx->prm.accum_depth_min_m; p.zmax = (float)ctx->prm.accum_depth_max_m;
    p.w = w; p.h = h; p.min_kpts = ctx->prm.accum_min_kpts; p.silence_ok = silence_ok;
    p.L = db.records; p.T = db.rows;
    auto kern = cam.lens() ? k_accumulate<true, KPD> : k_accumulate<false, KPD>;
    hipLaunchKernelGGL(kern, dim3(1), dim3(1024), 0, ctx->stream, ctx->orb.buf.f_xy, ctx->orb.buf.f_desc, ctx->orb.buf.f_count, ctx->max_feat,
                       depth_mm_dev, w, p, ctx->tick.res, db.xy_heading, db.desc, db.pts3d, db.kp2d, db.off, db.pose, ctx->accum_res,
                       make_dist(cam.lens()));
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

RELOC_API int reloc_tick_accumulate_dev(reloc_ctx *ctx, const uint16_t *depth_mm_dev, int w, int h, const double base_pose[7],
                                        int silence_ok)
{
    ARG_CHECK_CTX(ctx, depth_mm_dev && base_pose && w >= 64 && h >= 64, "reloc_tick_accumulate_dev");
    if (int rc = accum_reserve(ctx)) return rc;
    if (int rc = image_chain_depth(ctx, depth_mm_dev, &w, &h, &depth_mm_dev)) return rc;      // from here on the working frame
    return accum_launch<false>(ctx, depth_mm_dev, w, h, base_pose, silence_ok);
}

// the same with the depth of the tick's keypoints from the right eye's frame (include/reloc_spec.h "STEREO"); enqueues only
RELOC_API int reloc_tick_accumulate_stereo_dev(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *img_right_dev, int w, int h, int order,
                                               const double base_pose[7], int silence_ok)
{
    ARG_CHECK_CTX(ctx, right && img_right_dev && base_pose && w >= 64 && h >= 64, "reloc_tick_accumulate_stereo_dev");
    if (!ctx->stereo.on()) { reloc_set_error("stereo is off on this context (reloc_set_stereo)"); return RELOC_E_STATE; }
    if (int rc = accum_reserve(ctx)) return rc;
    if (int rc = stereo_frame(ctx, right, img_right_dev, w, h, order, &w, &h)) return rc;      // from here on the working frame
    return accum_launch<true>(ctx, ctx->stereo.mm, w, h, base_pose, silence_ok);
}

RELOC_API int reloc_accumulate_result(reloc_ctx *ctx, int32_t *appended, int32_t *n_kpts, double *nearest_m)
{
    ARG_CHECK_CTX(ctx, true, "ctx is NULL");
    AccumResult r;
    HIP_TRY(hipMemcpyAsync(&r, ctx->accum_res, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (r.appended == 1) {
        // adopt the record the kernel wrote behind the last row; exactly once per accumulate call
        DbArena &db = ctx_db(ctx);
        db.records += 1;
        db.rows += r.n_kpts;
        if (r.n_kpts > db.max_rows) db.max_rows = r.n_kpts;
        const int32_t zero = 0;
        HIP_TRY(hipMemcpyAsync(&ctx->accum_res->appended, &zero, 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (appended) *appended = r.appended;
    if (n_kpts) *n_kpts = r.n_kpts;
    if (nearest_m) *nearest_m = r.nearest_m;
    return RELOC_OK;
}

// ---------------------------------------------------------------------------------------------------
// Depth image -> obstacle point cloud (reference relay depth_cb,
// tf_wall_clock_relay_v55.py:1020-1038): every `step`-th pixel, keep 0.3 < z < 10 and finite,
// point = (z, -(u - cx) / fx * z, -(v - cy) / fy * z) in float32, raster order.
__global__ __launch_bounds__(1024) void k_depth_points(DepthGrid g, float *__restrict__ out, int32_t *__restrict__ o_n)
{
    __shared__ int s_wsum[16];
    const int tid = threadIdx.x;
    const int n = g.cols() * g.rows();
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        float p[3];
        const bool keep = i < n && depth_grid_point(g, g.is_f32 != 0, i, p);
        int total;
        const int pos = block_rank(keep, s_wsum, base, total);
        if (keep) { out[3 * pos] = p[0]; out[3 * pos + 1] = p[1]; out[3 * pos + 2] = p[2]; }
        base += total;
    }
    if (tid == 0) *o_n = base;
}

// The cloud of a depth plane on the device into the caller's points (room for cols x rows rows of 3 floats): scratch slot 6,
// k_depth_points, the count, then the rows.  Returns the rows, 0 after an error.
static int32_t depth_cloud(HostStaging &st, const DepthGrid &g, float *points)
{
    const int64_t cap = (int64_t)g.cols() * g.rows();
    float *dout = st.slot<float>(6, cap * 3 + 4);
    if (st.rc) return 0;
    int32_t *o_n = (int32_t *)(dout + cap * 3);
    st.launch(k_depth_points, dim3(1), dim3(1024), g, dout, o_n);
    const int32_t n = st.count(o_n);
    if (n > 0) st.download(points, dout, (int64_t)n * 12);
    return n;
}

// depth: (h, w) float32 metres (is_f32 = 1) or uint16 millimetres (is_f32 = 0), dense rows.
// points must hold ceil(w/step) * ceil(h/step) rows of 3 floats.
RELOC_API int reloc_depth_points(reloc_ctx *ctx, const void *depth, int is_f32, int w, int h, int step, const double K4[4],
                                 float zmin, float zmax, float *points, int32_t *n_out)
{
    ARG_CHECK_CTX(ctx, depth && points && n_out && w > 0 && h > 0 && step > 0 && K4, "reloc_depth_points");
    HostStaging st{ctx};
    const int32_t n = depth_cloud(st, frame_from_depth(st, depth, is_f32, w, h, step, K4, zmin, zmax).src.grid, points);
    if (int rc = st.finish()) return rc;
    *n_out = n;
    return RELOC_OK;
}

// The cloud of a stereo pair: the dense pass of reloc_stereo_dense.hip, then k_depth_points on its plane where it lies.
RELOC_API int reloc_stereo_frame_points(reloc_ctx *ctx, reloc_ctx *right, const uint8_t *img, const uint8_t *img_right, int w, int h,
                                        int order, int step, float zmin, float zmax, float *points, int32_t *n_out)
{
    ARG_CHECK_CTX(ctx, right && img && img_right && points && n_out && w >= 64 && h >= 64 && step > 0, "reloc_stereo_frame_points");
    if (int rc = stereo_pair_entry(ctx, right, w, h)) return rc;
    *n_out = 0;
    StereoPairStaging st(ctx, right);
    st.upload_pair(img, img_right, w, h);
    st.run([&] { return stereo_dense_frame(ctx, right, w, h, order, &w, &h); });      // from here on the working frame
    const int32_t n = depth_cloud(st, frame_from_stereo(st, step, zmin, zmax).src.grid, points);      // the pass just enqueued
    if (int rc = st.finish()) return rc;
    *n_out = n;
    return RELOC_OK;
}
