// reloc_db.hip -- the resident landmark databases of a context: two slots of one DbArena each (reloc_internal.h).
//
// A database is a capacity-reserved arena: upload fills it, append copies one record behind the last row, reserve grows
// it, share adopts another context's arrays by reference count, select switches between the two slots.  The arena is the
// unit of ownership.  There is one way into a slot -- a complete arena, built aside, is assigned to it -- and one way out,
// db_arena_release.  Nothing is published in the ctx before every allocation and copy of an operation has succeeded: a
// failed upload leaves "no database" (records == 0), a failed reserve / append leaves the database as it was.
// The scans of a database are in reloc_scan.hip, reloc_scan_rows.hip and reloc_ratio.hip, the appending kernel of the fused tick in reloc_record.hip.
#include <new>

#include "reloc_internal.h"

// (cos, sin) of the heading of base_link +X in the world from the stored CAMERA pose of record i, exactly as the
// reference composes it (M:233-245): R_wb = R_wc @ B.T, fwd = R_wb @ [1,0,0] = R_wc @ B[0,:]
__device__ __forceinline__ void record_heading(const double *__restrict__ pose, int64_t i, double b0, double b1, double b2,
                                               double &ch, double &sh)
{
    const double qx = pose[7 * i + 3], qy = pose[7 * i + 4], qz = pose[7 * i + 5], qw = pose[7 * i + 6];
    const double r00 = 1 - 2 * (qy * qy + qz * qz), r01 = 2 * (qx * qy - qz * qw), r02 = 2 * (qx * qz + qy * qw);
    const double r10 = 2 * (qx * qy + qz * qw), r11 = 1 - 2 * (qx * qx + qz * qz), r12 = 2 * (qy * qz - qx * qw);
    const double fx = r00 * b0 + r01 * b1 + r02 * b2, fy = r10 * b0 + r11 * b1 + r12 * b2;
    const double fn = sqrt(fx * fx + fy * fy);
    ch = fn > 0 ? fx / fn : 1.0;
    sh = fn > 0 ? fy / fn : 0.0;
}

// index entries (x, y, cos heading, sin heading) of records first .. first + n - 1
__global__ void k_db_index(const double *__restrict__ pose, int64_t first, int64_t n, double b0, double b1, double b2,
                           double *__restrict__ xyh)
{
    const int64_t i = first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= first + n) return;
    double ch, sh;
    record_heading(pose, i, b0, b1, b2, ch, sh);
    xyh[4 * i] = pose[7 * i];
    xyh[4 * i + 1] = pose[7 * i + 1];
    xyh[4 * i + 2] = ch;
    xyh[4 * i + 3] = sh;
}

// headings follow the camera mounting (reloc_set_camera); the (x, y) a record is filed under is kept
__global__ void k_db_reheading(const double *__restrict__ pose, int64_t n, double b0, double b1, double b2, double *__restrict__ xyh)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double ch, sh;
    record_heading(pose, i, b0, b1, b2, ch, sh);
    xyh[4 * i + 2] = ch;
    xyh[4 * i + 3] = sh;
}

int db_reindex(reloc_ctx *ctx)
{
    // both resident databases follow a change of the camera mounting
    for (const DbArena &db : ctx->db_slot) {
        if (!db.pose || !db.xy_heading || db.records <= 0) continue;
        hipLaunchKernelGGL(k_db_reheading, dim3((unsigned)((db.records + 255) / 256)), dim3(256), 0, ctx->stream, db.pose, db.records,
                           ctx->cam.b2c_R[0], ctx->cam.b2c_R[1], ctx->cam.b2c_R[2], db.xy_heading);
    }
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

void db_arena_release(DbArena &a)
{
    if (a.share && __atomic_sub_fetch(&a.share->refs, 1, __ATOMIC_ACQ_REL) == 0) {
        void *p[] = {a.desc, a.pts3d, a.kp2d, a.off, a.pose, a.xy_heading};
        for (void *q : p) if (q) (void)hipFree(q);
        delete a.share;
    }
    if (a.counts) (void)hipFree(a.counts);
    if (a.topk_part) (void)hipFree(a.topk_part);
    a = DbArena();
}

// Grow the selected arena to at least (cap_records, cap_rows); contents are kept.  All-or-nothing: the new arena is built
// aside and replaces the old one when it is complete.  The old arrays are let go of, not necessarily freed: contexts that
// adopted them (reloc_db_share) keep scanning them.
int db_reserve(reloc_ctx *ctx, int64_t cap_records, int64_t cap_rows)
{
    DbArena &db = ctx_db(ctx);
    if (db.shared) { reloc_set_error("the selected database is shared from another context (read-only here)"); return RELOC_E_STATE; }
    if (cap_records < 1) cap_records = 1;
    if (cap_rows < 1) cap_rows = 1;
    if (cap_records <= db.cap_records && cap_rows <= db.cap_rows && db.desc) return RELOC_OK;
    if (cap_records < db.cap_records) cap_records = db.cap_records;
    if (cap_rows < db.cap_rows) cap_rows = db.cap_rows;
    if (cap_records > MAX_DB_RECORDS) { reloc_set_error("database: more than %lld records", (long long)MAX_DB_RECORDS); return RELOC_E_CAPACITY; }
    DbArena nb;                        // its only holder until it is assigned: db_arena_release(nb) frees all of it
    nb.share = new (std::nothrow) DbShare();
    if (!nb.share) { reloc_set_error("database reserve: out of host memory"); return RELOC_E_HIP; }
    nb.cap_records = cap_records;
    nb.cap_rows = cap_rows;
    nb.topk_blocks = (int)((cap_records + 1023) / 1024);
    hipError_t e = hipSuccess;
    auto grab = [&](void **p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    grab((void **)&nb.desc, (size_t)cap_rows * 32);
    grab((void **)&nb.pts3d, (size_t)cap_rows * 12);
    grab((void **)&nb.kp2d, (size_t)cap_rows * 8);
    grab((void **)&nb.off, (size_t)(cap_records + 1) * 8);
    grab((void **)&nb.pose, (size_t)cap_records * 56);
    grab((void **)&nb.xy_heading, (size_t)cap_records * 32);
    grab((void **)&nb.counts, (size_t)cap_records * 4);
    grab((void **)&nb.topk_part, (size_t)nb.topk_blocks * 32 * sizeof(unsigned long long));
    const int64_t L = db.desc ? db.records : 0, T = db.desc ? db.rows : 0;
    auto copy = [&](void *d, const void *s_, size_t bytes) {
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(d, s_, bytes, hipMemcpyDeviceToDevice, ctx->stream);
    };
    if (L > 0) {
        copy(nb.desc, db.desc, (size_t)T * 32);
        copy(nb.pts3d, db.pts3d, (size_t)T * 12);
        copy(nb.kp2d, db.kp2d, (size_t)T * 8);
        copy(nb.off, db.off, (size_t)(L + 1) * 8);
        copy(nb.pose, db.pose, (size_t)L * 56);
        copy(nb.xy_heading, db.xy_heading, (size_t)L * 32);
    } else if (e == hipSuccess) {
        e = hipMemsetAsync(nb.off, 0, 8, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        db_arena_release(nb);
        (void)hipGetLastError();          // a failed hipMalloc leaves a sticky error that the next launch check would report
        reloc_set_error("database reserve (%lld records, %lld rows) failed: %s", (long long)cap_records, (long long)cap_rows,
                        hipGetErrorString(e));
        return RELOC_E_HIP;
    }
    nb.records = L;
    nb.rows = T;
    nb.max_rows = db.max_rows;
    db_arena_release(db);
    db = nb;
    return RELOC_OK;
}

RELOC_API int reloc_db_reserve(reloc_ctx *ctx, int64_t cap_records, int64_t cap_rows)
{
    ARG_CHECK_CTX(ctx, cap_records >= 0 && cap_rows >= 0, "reloc_db_reserve");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return db_reserve(ctx, cap_records, cap_rows);
}

RELOC_API int reloc_db_upload(reloc_ctx *ctx, const uint8_t *desc, const float *pts3d, const int64_t *offsets,
                              const double *poses, int64_t n_records)
{
    ARG_CHECK_CTX(ctx, offsets && n_records >= 0, "reloc_db_upload");
    const int64_t T = offsets[n_records];
    ARG_CHECK(offsets[0] == 0 && T >= 0, "offsets must start at 0 and be non-decreasing");
    int maxrows = 0;
    for (int64_t r = 0; r < n_records; ++r) {
        const int64_t n = offsets[r + 1] - offsets[r];
        ARG_CHECK(n >= 0, "offsets must be non-decreasing");
        if (n > MAX_REC_ROWS) { reloc_set_error("record %lld has %lld rows (max %d)", (long long)r, (long long)n, MAX_REC_ROWS); return RELOC_E_CAPACITY; }
        if (n > maxrows) maxrows = (int)n;
    }
    ARG_CHECK(T == 0 || (desc && pts3d), "desc / pts3d missing");
    ARG_CHECK(n_records == 0 || poses, "poses missing");
    if (n_records > MAX_DB_RECORDS) { reloc_set_error("database: %lld records (max %lld)", (long long)n_records, (long long)MAX_DB_RECORDS); return RELOC_E_CAPACITY; }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    DbArena &db = ctx_db(ctx);
    // arrays adopted from another context, or adopted by others, are let go of: whoever else holds them keeps them as they
    // are, this upload goes into fresh ones
    if (db.shared || (db.share && __atomic_load_n(&db.share->refs, __ATOMIC_ACQUIRE) > 1)) db_arena_release(db);
    // from here on the ctx holds no database until everything below has succeeded
    db.records = 0;
    db.rows = 0;
    db.max_rows = 0;
    int rc = db_reserve(ctx, n_records, T);
    if (rc) return rc;
    if (T > 0) {
        HIP_TRY(hipMemcpyAsync(db.desc, desc, (size_t)T * 32, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(db.pts3d, pts3d, (size_t)T * 12, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemsetAsync(db.kp2d, 0, (size_t)T * 8, ctx->stream));
    }
    HIP_TRY(hipMemcpyAsync(db.off, offsets, (size_t)(n_records + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (n_records > 0) {
        HIP_TRY(hipMemcpyAsync(db.pose, poses, (size_t)n_records * 56, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_db_index, dim3((unsigned)((n_records + 255) / 256)), dim3(256), 0, ctx->stream, db.pose, (int64_t)0,
                           n_records, ctx->cam.b2c_R[0], ctx->cam.b2c_R[1], ctx->cam.b2c_R[2], db.xy_heading);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    db.records = n_records;
    db.rows = T;
    db.max_rows = maxrows;
    return RELOC_OK;
}

// room for one more record of n rows; geometric growth when the reserve is exhausted
static int db_make_room(reloc_ctx *ctx, int64_t n)
{
    const DbArena &db = ctx_db(ctx);
    if (db.desc && db.records + 1 <= db.cap_records && db.rows + n <= db.cap_rows) return RELOC_OK;
    const int64_t need_r = db.records + 1, need_t = db.rows + n;
    int64_t cr = db.cap_records + db.cap_records / 2 + 64, ct = db.cap_rows + db.cap_rows / 2 + 64 * 512;
    if (cr < need_r) cr = need_r;
    if (ct < need_t) ct = need_t;
    if (cr > MAX_DB_RECORDS) cr = MAX_DB_RECORDS;
    if (need_r > MAX_DB_RECORDS) { reloc_set_error("database: more than %lld records", (long long)MAX_DB_RECORDS); return RELOC_E_CAPACITY; }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return db_reserve(ctx, cr, ct);
}

RELOC_API int reloc_db_append(reloc_ctx *ctx, const uint8_t *desc, const float *pts3d, const float *kp2d, int n,
                              const double pose[7], const double index_xy[2])
{
    ARG_CHECK_CTX(ctx, n >= 0 && pose && (n == 0 || (desc && pts3d)), "reloc_db_append");
    DbArena &db = ctx_db(ctx);
    if (db.shared) { reloc_set_error("the selected database is shared from another context (read-only here)"); return RELOC_E_STATE; }
    if (n > MAX_REC_ROWS) { reloc_set_error("record has %d rows (max %d)", n, MAX_REC_ROWS); return RELOC_E_CAPACITY; }
    int rc = db_make_room(ctx, n);
    if (rc) return rc;
    const int64_t L = db.records, T = db.rows;
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(db.desc + T * 32, desc, (size_t)n * 32, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(db.pts3d + T * 3, pts3d, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
        if (kp2d) HIP_TRY(hipMemcpyAsync(db.kp2d + T * 2, kp2d, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
        else HIP_TRY(hipMemsetAsync(db.kp2d + T * 2, 0, (size_t)n * 8, ctx->stream));
    }
    const int64_t end = T + n;
    HIP_TRY(hipMemcpyAsync(db.off + L + 1, &end, 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(db.pose + 7 * L, pose, 56, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_db_index, dim3(1), dim3(64), 0, ctx->stream, db.pose, L, (int64_t)1, ctx->cam.b2c_R[0], ctx->cam.b2c_R[1],
                       ctx->cam.b2c_R[2], db.xy_heading);
    HIP_TRY(hipGetLastError());
    if (index_xy) HIP_TRY(hipMemcpyAsync(db.xy_heading + 4 * L, index_xy, 16, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));     // the host sources may go away; the record is visible from here on
    db.records = L + 1;
    db.rows = end;
    if (n > db.max_rows) db.max_rows = n;
    return RELOC_OK;
}

RELOC_API int reloc_db_share(reloc_ctx *dst, reloc_ctx *src)
{
    ARG_CHECK_CTX(dst, src && src != dst, "reloc_db_share");
    if (src->device != dst->device) { reloc_set_error("reloc_db_share: contexts live on different devices"); return RELOC_E_ARG; }
    if (!db_ready(src)) { reloc_set_error("reloc_db_share: the source context has no database"); return RELOC_E_STATE; }
    HIP_TRY(hipStreamSynchronize(dst->stream));
    HIP_TRY(hipStreamSynchronize(src->stream));
    // the adopter's arena: the source's arrays, counters and capacities as they are now, scratch of its own
    DbArena nb = ctx_db(src);
    nb.shared = true;
    nb.counts = nullptr;
    nb.topk_part = nullptr;
    if (hipMalloc((void **)&nb.counts, (size_t)nb.cap_records * 4) != hipSuccess ||
        hipMalloc((void **)&nb.topk_part, (size_t)nb.topk_blocks * 32 * sizeof(unsigned long long)) != hipSuccess) {
        if (nb.counts) (void)hipFree(nb.counts);
        reloc_set_error("reloc_db_share: scratch allocation failed");
        return RELOC_E_HIP;
    }
    __atomic_add_fetch(&nb.share->refs, 1, __ATOMIC_ACQ_REL);
    DbArena &db = ctx_db(dst);
    db_arena_release(db);
    db = nb;
    return RELOC_OK;
}

RELOC_API int reloc_db_select(reloc_ctx *ctx, int slot)
{
    ARG_CHECK_CTX(ctx, slot == 0 || slot == 1, "reloc_db_select: slot must be 0 or 1");
    if (slot == ctx->db_sel) return RELOC_OK;
    if (ctx_db(ctx).shared) { reloc_set_error("reloc_db_select: the selected database is shared; upload or share per slot instead"); return RELOC_E_STATE; }
    ctx->db_sel = slot;
    return RELOC_OK;
}

RELOC_API int reloc_db_fetch(reloc_ctx *ctx, int64_t record, uint8_t *desc, float *pts3d, float *kp2d, double pose[7],
                             double index_xyh[4], int32_t *n)
{
    ARG_CHECK_CTX(ctx, record >= 0, "reloc_db_fetch");
    const DbArena &db = ctx_db(ctx);
    if (!db_ready(ctx) || record >= db.records) { reloc_set_error("db fetch: record %lld of %lld", (long long)record, (long long)db.records); return RELOC_E_STATE; }
    int64_t o[2];
    HIP_TRY(hipMemcpyAsync(o, db.off + record, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const int64_t cnt = o[1] - o[0];
    if (n) *n = (int32_t)cnt;
    if (cnt > 0) {
        if (desc) HIP_TRY(hipMemcpyAsync(desc, db.desc + o[0] * 32, (size_t)cnt * 32, hipMemcpyDeviceToHost, ctx->stream));
        if (pts3d) HIP_TRY(hipMemcpyAsync(pts3d, db.pts3d + o[0] * 3, (size_t)cnt * 12, hipMemcpyDeviceToHost, ctx->stream));
        if (kp2d) HIP_TRY(hipMemcpyAsync(kp2d, db.kp2d + o[0] * 2, (size_t)cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (pose) HIP_TRY(hipMemcpyAsync(pose, db.pose + 7 * record, 56, hipMemcpyDeviceToHost, ctx->stream));
    if (index_xyh) HIP_TRY(hipMemcpyAsync(index_xyh, db.xy_heading + 4 * record, 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RELOC_OK;
}

RELOC_API int64_t reloc_db_records(reloc_ctx *ctx) { return ctx ? ctx_db(ctx).records : -1; }
RELOC_API int64_t reloc_db_rows(reloc_ctx *ctx) { return ctx ? ctx_db(ctx).rows : -1; }
RELOC_API int32_t *reloc_db_counts_dev(reloc_ctx *ctx) { return ctx && db_ready(ctx) ? ctx_db(ctx).counts : nullptr; }
