// reloc_ctx.hip -- context lifetime, error reporting, stream/event plumbing of libreloc_hip.so.
#include <stdarg.h>
#include <stdlib.h>

#include "reloc_internal.h"

static thread_local char g_err[512] = "";

void reloc_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

RELOC_API const char *reloc_last_error(void) { return g_err; }

RELOC_API int reloc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int ctx_alloc(reloc_ctx *c)
{
    if (int rc = orb_alloc(c)) return rc;
    if (int rc = scan_alloc(c)) return rc;
    if (int rc = tick_alloc(c)) return rc;
    if (int rc = frame_img_reserve(c, 3)) return rc;
    return c->accum_block.layout(c, [&](BlockCarver &b) { b.own(c->accum_res, 1); });
}

int g_reloc_live_contexts = 0;

RELOC_API reloc_ctx *reloc_create(int device, int max_w, int max_h, int max_feat)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        reloc_set_error("no HIP device available (libreloc_hip has no CPU fallback)");
        return nullptr;
    }
    if (device < 0 || device >= n || max_w < 64 || max_h < 64 || max_feat < 64) {
        reloc_set_error("reloc_create: bad arguments (device %d of %d, %dx%d, max_feat %d)", device, n,
                        max_w, max_h, max_feat);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        reloc_set_error("hipSetDevice(%d) failed", device);
        return nullptr;
    }
    reloc_ctx *c = new reloc_ctx();
    __atomic_add_fetch(&g_reloc_live_contexts, 1, __ATOMIC_RELAXED);     // reloc_destroy (also the failure paths below) takes it back
    c->device = device;
    c->max_w = max_w;
    c->max_h = max_h;
    c->max_feat = max_feat;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->t0) != hipSuccess || hipEventCreate(&c->t1) != hipSuccess) {
        reloc_set_error("stream/event creation failed");
        __atomic_sub_fetch(&g_reloc_live_contexts, 1, __ATOMIC_RELAXED);
        delete c;
        return nullptr;
    }
    c->stream = c->own_stream;
    // reference constants (include/reloc_spec.h); reloc_set_params overrides them
    c->prm.nfeatures = 500;
    c->prm.max_candidates = RELOC_MAX_CANDIDATES;
    c->prm.min_matches = RELOC_MIN_MATCHES;
    c->prm.min_inliers = RELOC_MIN_INLIERS;
    c->prm.ransac_iterations = RELOC_RANSAC_ITERATIONS;
    c->prm.global_max_candidates = RELOC_GLOBAL_MAX_CANDIDATES;
    c->prm.global_min_inliers = RELOC_GLOBAL_MIN_INLIERS;
    c->prm.accum_min_kpts = RELOC_ACCUM_MIN_KPTS;
    c->prm.candidate_radius_m = RELOC_CANDIDATE_RADIUS_M;
    c->prm.heading_tol_deg = RELOC_HEADING_TOL_DEG;
    c->prm.reproj_max_px = RELOC_REPROJ_MAX_PX;
    c->prm.ransac_reproj_px = RELOC_RANSAC_REPROJ_PX;
    c->prm.ransac_confidence = RELOC_RANSAC_CONFIDENCE;
    c->prm.consistency_m = RELOC_CONSISTENCY_M;
    c->prm.global_reproj_max_px = RELOC_GLOBAL_REPROJ_MAX_PX;
    c->prm.accum_min_dist_m = RELOC_ACCUM_MIN_DIST_M;
    c->prm.accum_depth_min_m = RELOC_ACCUM_DEPTH_MIN_M;
    c->prm.accum_depth_max_m = RELOC_ACCUM_DEPTH_MAX_M;
    c->prm.gray_coeff_bits = RELOC_GRAY_DEFAULT_BITS;     // OpenCV 4.x set (reloc_spec.h)
    c->prm.reserved0 = 0;
    // Developer switches (tools/exp_*, one test): read ONLY when RELOC_DEV=1 is set, once, here.  A deployment's environment
    // cannot change the library's behaviour by accident; none of them changes a result.
    if (const char *dev = getenv("RELOC_DEV"); dev && dev[0] == '1' && dev[1] == 0) {
        if (const char *e = getenv("RELOC_SCAN_GENS")) c->scan_gens = atoi(e);
        if (const char *e = getenv("RELOC_LOCAL_TWO_STAGE")) c->local_two_stage = atoi(e) != 0;
    }
    if (ctx_alloc(c) != 0) {
        reloc_destroy(c);
        return nullptr;
    }
    return c;
}

RELOC_API void reloc_destroy(reloc_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (DbArena &db : c->db_slot) db_arena_release(db);      // owner or adopter alike: one reference each
    tick_release(c);
    stereo_release(c);
    obs_release(c);
    for (int k = 0; k < RELOC_PROF_COUNT; ++k)
        if (c->prof[k].init)
            for (int i = 0; i < RELOC_PROF_RING; ++i) {
                (void)hipEventDestroy(c->prof[k].a[i]);
                (void)hipEventDestroy(c->prof[k].b[i]);
            }
    if (c->t0) (void)hipEventDestroy(c->t0);
    if (c->t1) (void)hipEventDestroy(c->t1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    __atomic_sub_fetch(&g_reloc_live_contexts, 1, __ATOMIC_RELAXED);
    delete c;      // the device blocks go with their owners (DevBlock): the device is current and the stream drained
}

RELOC_API int reloc_get_params(reloc_ctx *c, reloc_params *out)
{
    ARG_CHECK_CTX(c, out, "reloc_get_params");
    *out = c->prm;
    return RELOC_OK;
}

RELOC_API int reloc_set_params(reloc_ctx *c, const reloc_params *p)
{
    ARG_CHECK_CTX(c, p, "reloc_set_params");
    ARG_CHECK(p->nfeatures >= 1 && p->nfeatures <= c->max_feat, "nfeatures must be in [1, max_feat]");
    ARG_CHECK(p->max_candidates >= 1 && p->max_candidates * 3 <= 32, "max_candidates must be in [1, 10]");
    ARG_CHECK(p->global_max_candidates >= 1 && p->global_max_candidates <= MAX_CAND, "global_max_candidates must be in [1, 32]");
    ARG_CHECK(p->ransac_iterations >= 1 && p->ransac_iterations <= MAX_HYP, "ransac_iterations must be in [1, 1024]");
    ARG_CHECK(p->min_matches >= RELOC_PNP_SAMPLE && p->min_inliers >= 0 && p->global_min_inliers >= 0 && p->accum_min_kpts >= 1,
              "min_matches must be >= 4, inlier / keypoint gates non-negative");
    ARG_CHECK(p->candidate_radius_m >= 0 && p->heading_tol_deg >= 0 && p->heading_tol_deg <= 180 && p->ransac_reproj_px > 0 &&
                  p->ransac_confidence > 0 && p->ransac_confidence < 1 && p->consistency_m >= 0 && p->accum_min_dist_m >= 0,
              "a gate is out of range");
    ARG_CHECK((p->gray_coeff_bits == RELOC_GRAY_SHIFT || p->gray_coeff_bits == RELOC_GRAY15_SHIFT) && p->reserved0 == 0,
              "gray_coeff_bits must be 14 or 15, reserved0 must be 0");
    c->prm = *p;
    return RELOC_OK;
}

RELOC_API int reloc_set_stream(reloc_ctx *c, void *hip_stream)
{
    ARG_CHECK_CTX(c, true, "ctx is NULL");
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return RELOC_OK;
}

RELOC_API int reloc_sync(reloc_ctx *c)
{
    ARG_CHECK_CTX(c, true, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RELOC_OK;
}

RELOC_API void *reloc_dev_alloc(reloc_ctx *c, int64_t bytes)
{
    if (!c || bytes < 0) { reloc_set_error("reloc_dev_alloc: bad arguments"); return nullptr; }
    void *p = nullptr;
    (void)hipSetDevice(c->device);
    if (hipMalloc(&p, (size_t)(bytes > 0 ? bytes : 1)) != hipSuccess) {
        reloc_set_error("hipMalloc(%lld) failed", (long long)bytes);
        return nullptr;
    }
    return p;
}

RELOC_API int reloc_dev_free(reloc_ctx *c, void *p)
{
    ARG_CHECK_CTX(c, true, "ctx is NULL");
    if (p) HIP_TRY(hipFree(p));
    return RELOC_OK;
}

RELOC_API int reloc_h2d(reloc_ctx *c, void *dst, const void *src, int64_t bytes)
{
    ARG_CHECK_CTX(c, dst && src && bytes >= 0, "reloc_h2d");
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    return RELOC_OK;
}

RELOC_API int reloc_d2d(reloc_ctx *c, void *dst, const void *src, int64_t bytes)
{
    ARG_CHECK_CTX(c, dst && src && bytes >= 0, "reloc_d2d");
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, c->stream));
    return RELOC_OK;
}

RELOC_API int reloc_set_exclusive(reloc_ctx *c, int on)
{
    ARG_CHECK_CTX(c, true, "ctx is NULL");
    c->exclusive_hint = on < 0 ? -1 : (on != 0);
    return RELOC_OK;
}

RELOC_API void *reloc_host_alloc(int64_t bytes)
{
    void *p = nullptr;
    if (bytes < 0 || hipHostMalloc(&p, (size_t)(bytes > 0 ? bytes : 1), hipHostMallocDefault) != hipSuccess) {
        reloc_set_error("hipHostMalloc(%lld) failed", (long long)bytes);
        return nullptr;
    }
    return p;
}

RELOC_API int reloc_host_free(void *p)
{
    if (p) HIP_TRY(hipHostFree(p));
    return RELOC_OK;
}

RELOC_API void *reloc_get_stream(reloc_ctx *c) { return c ? (void *)c->stream : nullptr; }

RELOC_API int reloc_d2h(reloc_ctx *c, void *dst, const void *src, int64_t bytes)
{
    ARG_CHECK_CTX(c, dst && src && bytes >= 0, "reloc_d2h");
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    return RELOC_OK;
}

RELOC_API int reloc_timer_begin(reloc_ctx *c)
{
    ARG_CHECK_CTX(c, true, "ctx is NULL");
    HIP_TRY(hipEventRecord(c->t0, c->stream));
    return RELOC_OK;
}

RELOC_API int reloc_timer_end(reloc_ctx *c, float *ms)
{
    ARG_CHECK_CTX(c, ms, "reloc_timer_end");
    HIP_TRY(hipEventRecord(c->t1, c->stream));
    HIP_TRY(hipEventSynchronize(c->t1));
    HIP_TRY(hipEventElapsedTime(ms, c->t0, c->t1));
    return RELOC_OK;
}

// ---- staging of the host-pointer entry points (HostStaging, reloc_internal.h) -----------------------------------
void *HostStaging::slot_bytes(int s, int64_t bytes)
{
    DevBlock &b = ctx->scratch[s];
    if (!rc && (int64_t)b.bytes < bytes) rc = b.reserve(ctx, (size_t)(bytes + bytes / 4 + 4096));
    return rc ? nullptr : b.p;
}

// ---- the one owner of a context's device memory (DevBlock, reloc_internal.h) ---------------------------------------------
int DevBlock::reserve(reloc_ctx *ctx, size_t need, size_t keep)
{
    if (p && bytes >= need) return RELOC_OK;
    uint8_t *grown = nullptr;
    if (hipError_t e = hipMalloc((void **)&grown, need ? need : 1); e != hipSuccess) {
        (void)hipGetLastError();      // the context lives on with the old block: no sticky error for its next launch check
        reloc_set_error("hipMalloc(%zu) failed: %s", need, hipGetErrorString(e));
        return RELOC_E_HIP;
    }
    if (p) {
        hipError_t e = hipStreamSynchronize(ctx->stream);      // work in flight may still use the old block
        if (e == hipSuccess && keep) e = hipMemcpy(grown, p, keep, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            (void)hipFree(grown);
            reloc_set_error("growing a device block failed: %s", hipGetErrorString(e));
            return RELOC_E_HIP;
        }
        (void)hipFree(p);
    }
    p = grown;
    bytes = need;
    return RELOC_OK;
}

void DevBlock::release()
{
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}

void HostStaging::hip(hipError_t e, const char *what)
{
    if (rc || e == hipSuccess) return;
    reloc_set_error("%s failed: %s", what, hipGetErrorString(e));
    rc = RELOC_E_HIP;
}

// ---- per-kernel HIP-event stopwatch ----------------------------------------------------------
static void prof_flush(reloc_ctx *c, int which)
{
    auto &p = c->prof[which];
    for (int i = 0; i < p.n; ++i) {
        float ms = 0.f;
        if (hipEventSynchronize(p.b[i]) == hipSuccess && hipEventElapsedTime(&ms, p.a[i], p.b[i]) == hipSuccess) {
            p.total += ms;
            p.launches += 1;
        }
    }
    p.n = 0;
}

void reloc_prof_begin(reloc_ctx *c, int which)
{
    if (!c->prof_on) return;
    auto &p = c->prof[which];
    if (!p.init) {
        for (int i = 0; i < RELOC_PROF_RING; ++i) { (void)hipEventCreate(&p.a[i]); (void)hipEventCreate(&p.b[i]); }
        p.init = true;
    }
    if (p.n == RELOC_PROF_RING) prof_flush(c, which);
    (void)hipEventRecord(p.a[p.n], c->stream);
}

void reloc_prof_end(reloc_ctx *c, int which)
{
    if (!c->prof_on) return;
    auto &p = c->prof[which];
    (void)hipEventRecord(p.b[p.n], c->stream);
    p.n += 1;
}

RELOC_API int reloc_profile_enable(reloc_ctx *c, int on)
{
    ARG_CHECK_CTX(c, true, "ctx is NULL");
    for (int k = 0; k < RELOC_PROF_COUNT; ++k) {
        prof_flush(c, k);
        c->prof[k].total = 0.f;
        c->prof[k].launches = 0;
    }
    c->prof_on = on;
    return RELOC_OK;
}

RELOC_API int reloc_profile_get(reloc_ctx *c, int which, float *total_ms, int32_t *launches)
{
    ARG_CHECK_CTX(c, which >= 0 && which < RELOC_PROF_COUNT && total_ms && launches, "reloc_profile_get");
    prof_flush(c, which);
    *total_ms = c->prof[which].total;
    *launches = c->prof[which].launches;
    return RELOC_OK;
}
