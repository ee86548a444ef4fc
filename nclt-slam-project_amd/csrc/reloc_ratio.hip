// reloc_ratio.hip -- the Lowe-ratio match policy on gfx950 (CDNA4): knnMatch k=2 + ratio test (reference S:68-77) as the
// whole-database score (k_db_ratio, k_db_ratio_batch) and as the emit pass of the candidates (k_db_ratio_emit,
// k_db_ratio_emit_batch), with their launchers and the entry points that run them (reloc_db_ratio_counts, reloc_match_ratio).
// The crossCheck counterparts are in reloc_scan.hip, the primitives both use in reloc_hamming.h.
#include "reloc_hamming.h"

// ---------------------------------------------------------------------------------------------
// Ratio-test score of every record (reference _archive/anchor_localizer.py:82-90,
// checkpoint_a_selftest.py:68-71): per record, the number of current descriptors whose two nearest rows
// of the record satisfy d1 < ratio * d2.  Same data flow as k_db_scan (512 current descriptors per wave
// in registers, teach rows through the scalar cache) but the epilogue only tracks the two smallest
// distances per column: v_max_u16 + 2 v_min_u16 per pair, no indices, no cross-lane work in the loop.

// TICK: what scan_counts() needs of it under RELOC_MATCH_RATIO -- the heading mask and the AUTO stand-down of ScanMask, and the
// record-length gate (a record of fewer than min_rows rows is no candidate, S:64: count 0).  !TICK: reloc_db_ratio_counts, which
// reads none of the three.  Records are dealt statically: record r = block, + n_blocks, ...
template <bool TICK>
__device__ __forceinline__ void db_ratio_body(const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_rec,
                                              const uint4 *__restrict__ cur, int C, double ratio, int32_t *__restrict__ counts,
                                              const ScanMask &mask, int min_rows, int block, int n_blocks)
{
    __shared__ u32 s_part[4][512];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ncb = max((C + 511) >> 9, 1);
    double hc = 1.0, hs = 0.0, cos_tol = 0.0;
    if constexpr (TICK) {
        if (mask.skip_if && *mask.skip_if != 0) return;                  // RELOC_TICK_AUTO: the local search found candidates
        if (mask.xyh) {
            cur_heading_q(mask.q, hc, hs);
            hc = uniform_f64(hc); hs = uniform_f64(hs); cos_tol = uniform_f64(mask.cos_tol);
        }
    }
    u32 q[8][8];
    auto load_q = [&](int colbase) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int col = min(colbase + j * 64 + lane, max(C - 1, 0));
            const uint4 a = cur[2 * col], b = cur[2 * col + 1];
            q[j][0] = a.x; q[j][1] = a.y; q[j][2] = a.z; q[j][3] = a.w;
            q[j][4] = b.x; q[j][5] = b.y; q[j][6] = b.z; q[j][7] = b.w;
        }
    };
    if (ncb == 1 && C > 0) load_q(0);
    for (int r = block; r < n_rec; r += n_blocks) {
        const int64_t row0 = off[r];
        int n = (int)(off[r + 1] - row0);
        if constexpr (TICK) {
            if (n < min_rows || (mask.xyh && !heading_ok(mask.xyh + 4 * (int64_t)r, hc, hs, cos_tol))) n = 0;      // workgroup-uniform
        }
        const uint4 *rec = db + 2 * row0;
        int good = 0;
        if (n >= 2 && C > 0) {
            for (int cb = 0; cb < ncb; ++cb) {
                if (ncb > 1) load_q(cb * 512);
                u32 k0[8], k1[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) { k0[j] = 0xFFFFu; k1[j] = 0xFFFFu; }
                for (int t0 = wave * 8; t0 < n; t0 += 32) {
                    // rows through the scalar cache, one fetch in flight (see srow_landed); rows past the end
                    // re-read the last row and are skipped below, so a duplicate never counts twice
                    auto row_of = [&](int t) { return min(t0 + t, n - 1); };
                    uint4 a = rec[2 * row_of(0)], b = rec[2 * row_of(0) + 1];
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        srow_landed(a.x);
                        uint4 na, nb;
                        if (t + 1 < 8) { na = rec[2 * row_of(t + 1)]; nb = rec[2 * row_of(t + 1) + 1]; }
                        __builtin_amdgcn_sched_barrier(0);
                        if (t0 + t < n) {                                // wave-uniform
#pragma unroll
                            for (int j = 0; j < 8; j += 2) {
                                u32 h0, h1;
                                ham8x2(q[j], q[j + 1], a, b, 0, 0, h0, h1);
                                const u32 m0 = max_u16(k0[j], h0), m1 = max_u16(k0[j + 1], h1);
                                k0[j] = min_u16(k0[j], h0); k0[j + 1] = min_u16(k0[j + 1], h1);
                                k1[j] = min_u16(k1[j], m0); k1[j + 1] = min_u16(k1[j + 1], m1);
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        if (t + 1 < 8) { a = na; b = nb; }
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) s_part[wave][j * 64 + lane] = (k1[j] << 16) | k0[j];
                __syncthreads();
                for (int c = tid; c < 512; c += 256) {
                    u32 a0 = 0xFFFFu, a1 = 0xFFFFu;
                    for (int w = 0; w < 4; ++w) {
                        const u32 v = s_part[w][c];
                        const u32 lo = v & 0xFFFFu, hi = v >> 16;
                        // merge two sorted pairs: smallest two of {a0, a1, lo, hi}
                        const u32 n0 = a0 < lo ? a0 : lo;
                        const u32 n1 = a0 < lo ? (a1 < lo ? a1 : lo) : (hi < a0 ? hi : a0);
                        a0 = n0; a1 = n1;
                    }
                    const bool ok = cb * 512 + c < C && a1 != 0xFFFFu && (double)a0 < ratio * (double)a1;
                    good += __popcll(__ballot(ok));
                }
                __syncthreads();
            }
        }
        // every lane of a wave holds that wave's total; sum the four waves
        if (lane == 0) s_cnt[wave] = good;
        __syncthreads();
        if (tid == 0) counts[r] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        __syncthreads();
    }
}

template <bool TICK>
__global__ __launch_bounds__(256, 4) void k_db_ratio(const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_rec,
                                                     const uint4 *__restrict__ cur, const int32_t *__restrict__ n_cur_p,
                                                     int n_cur_max, double ratio, int32_t *__restrict__ counts, ScanMask mask,
                                                     int min_rows)
{
    const int C = cur_count(n_cur_p, n_cur_max);
    db_ratio_body<TICK>(db, off, n_rec, cur, C, ratio, counts, mask, min_rows, blockIdx.x, gridDim.x);
}

// the ratio scans of up to 8 frames in one launch: blockIdx.y = frame, which counts into bt.counts[frame] (ScanBatch)
__global__ __launch_bounds__(256, 4) void k_db_ratio_batch(const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_rec,
                                                           int n_cur_max, double ratio, ScanBatch bt, int min_rows)
{
    const int f = blockIdx.y;
    const ScanMask mask = scan_mask_of(bt, f);
    const int C = cur_count(bt.n_cur[f], n_cur_max);
    db_ratio_body<true>(db, off, n_rec, bt.cur[f], C, ratio, bt.counts[f], mask, min_rows, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------------------------------------
// The emit pass under RELOC_MATCH_RATIO (include/reloc_spec.h "MATCH POLICY"; S:68-77): the counterpart of k_db_scan_emit.  One
// workgroup of NW waves per candidate record, dealt statically; same EmitFrame buffers, so PnP and the finalisation run as
// they are.  The data flow is k_db_ratio's -- 64 x 8 current descriptors per wave in registers, the record's rows through the
// scalar cache with one fetch in flight, the waves of the workgroup splitting the rows 8 at a time -- but a column keeps its
// best KEY and its second best, key = distance << 22 | row: the minimum of keys is the smallest distance with the lowest row on
// ties, the second smallest key carries d2 (its row is not needed).  Per pair on top of the distance: v_lshl_or, v_max_u32,
// 2 v_min_u32.  The waves' partial pairs meet in LDS (NW x 512 x 2 words), a thread per column merges them, applies the test
// in double and the survivors are compacted by ballot in column (= queryIdx) order; the running base carries across the
// 64 * NW-column chunks and the 512-column blocks as db_emit_body's does across row blocks.
// m_n[it] = the list's length; gate_off > 0: m_n[gate_off + it] = the length PnP takes, 0 when the record has fewer than
// min_rows rows (the record-length gate of S:64, which a crossCheck list, never longer than its record, passes through the
// list-length gate alone).
constexpr int RATIO_KEY_SHIFT = 22;                 // rows of a record < 2^22, distances <= 256: keys < 0xFFFFFFFF = "none"
template <int NW>
__device__ __forceinline__ void db_ratio_emit_body(int C, const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_ids_max,
                                                   double ratio, int min_rows, int gate_off, int emit_stride,
                                                   const float *__restrict__ g_pts3d, const EmitFrame &F)
{
    static_assert(NW == 4 || NW == 8, "the two shapes launch_db_emit chooses between");
    __shared__ uint2 s_part[NW][512];
    __shared__ u32 s_wsum[NW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: row fetches stay scalar
    const int n_ids = F.n_ids_p ? min(*F.n_ids_p, n_ids_max) : n_ids_max;
    const int ncb = max((C + 511) >> 9, 1);
    const uint4 *__restrict__ cur = F.cur;
    u32 q[8][8];
    auto load_q = [&](int colbase) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int col = min(colbase + j * 64 + lane, max(C - 1, 0));   // padding repeats the last column, never listed
            const uint4 a = cur[2 * col], b = cur[2 * col + 1];
            q[j][0] = a.x; q[j][1] = a.y; q[j][2] = a.z; q[j][3] = a.w;
            q[j][4] = b.x; q[j][5] = b.y; q[j][6] = b.z; q[j][7] = b.w;
        }
    };
    if (ncb == 1 && C > 0) load_q(0);
    for (int it = blockIdx.x; it < n_ids; it += gridDim.x) {
        const int r = F.rec_ids ? F.rec_ids[it] : it;
        const int64_t row0 = off[r];
        const int n = (int)(off[r + 1] - row0);
        const uint4 *rec = db + 2 * row0;
        u32 base = 0;
        if (n >= 2 && C > 0) {
            for (int cb = 0; cb < ncb; ++cb) {
                if (ncb > 1) load_q(cb * 512);
                u32 k0[8], k1[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) { k0[j] = 0xFFFFFFFFu; k1[j] = 0xFFFFFFFFu; }
                for (int t0 = wave * 8; t0 < n; t0 += 8 * NW) {
                    // rows past the end re-read the last row and are skipped below (wave-uniform)
                    auto row_of = [&](int t) { return min(t0 + t, n - 1); };
                    uint4 a = rec[2 * row_of(0)], b = rec[2 * row_of(0) + 1];
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        srow_landed(a.x);
                        uint4 na, nb;
                        if (t + 1 < 8) { na = rec[2 * row_of(t + 1)]; nb = rec[2 * row_of(t + 1) + 1]; }
                        __builtin_amdgcn_sched_barrier(0);
                        if (t0 + t < n) {
                            const u32 w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                            u32 h[8];
                            ham8_cols<8>(q, w, h);                      // 8 accumulator chains, order pinned
                            const u32 row = (u32)(t0 + t);
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                const u32 key = (h[j] << RATIO_KEY_SHIFT) | row;
                                const u32 m = umax(k0[j], key);
                                k0[j] = umin(k0[j], key);
                                k1[j] = umin(k1[j], m);
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        if (t + 1 < 8) { a = na; b = nb; }
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) s_part[wave][j * 64 + lane] = make_uint2(k0[j], k1[j]);
                __syncthreads();
                for (int c0 = 0; c0 < 512 && cb * 512 + c0 < C; c0 += 64 * NW) {      // workgroup-uniform trip count
                    const int c = c0 + tid, col = cb * 512 + c;
                    // the two smallest keys of the waves' sorted pairs (keys of different waves name different rows)
                    u32 a0 = 0xFFFFFFFFu, a1 = 0xFFFFFFFFu;
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        const uint2 v = s_part[w][c];
                        const u32 n1 = umin(umax(a0, v.x), umin(a1, v.y));
                        a0 = umin(a0, v.x);
                        a1 = n1;
                    }
                    const u32 d1 = a0 >> RATIO_KEY_SHIFT, d2 = a1 >> RATIO_KEY_SHIFT;
                    const bool ok = col < C && a1 != 0xFFFFFFFFu && (double)d1 < ratio * (double)d2;
                    const unsigned long long bal = __ballot(ok);
                    if (lane == 0) s_wsum[wave] = (u32)__popcll(bal);
                    __syncthreads();
                    u32 before = base, total = 0;
                    for (int w = 0; w < NW; ++w) { const u32 x = s_wsum[w]; total += x; if (w < wave) before += x; }
                    if (ok) {
                        const u32 pos = before + (u32)__popcll(bal & ((1ull << lane) - 1ull));       // < C <= emit_stride
                        const u32 trow = a0 & ((1u << RATIO_KEY_SHIFT) - 1u);
                        const int64_t o = (int64_t)it * emit_stride + pos;
                        F.m_qidx[o] = col;
                        F.m_tidx[o] = (int32_t)trow;
                        F.m_dist[o] = (int32_t)d1;
                        if (F.g_obj) {
                            const float *p3 = g_pts3d + 3 * (row0 + trow), *p2 = F.g_xy + 2 * (size_t)col;
                            float *po = F.g_obj + 3 * o, *pi = F.g_img + 2 * o;
                            po[0] = p3[0]; po[1] = p3[1]; po[2] = p3[2];
                            pi[0] = p2[0]; pi[1] = p2[1];
                        }
                    }
                    base += total;
                    __syncthreads();                                    // s_wsum, and s_part of the next column block
                }
            }
        }
        if (tid == 0 && F.m_n) {
            F.m_n[it] = (int32_t)base;
            if (gate_off > 0) F.m_n[gate_off + it] = n >= min_rows ? (int32_t)base : 0;
        }
    }
}

// NW = 8 where nothing scans beside it (latency), 4 in ticks that scan the database: launch_db_emit's reasons
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_db_ratio_emit(const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_ids_max,
                                                           int n_cur_max, double ratio, int min_rows, int gate_off, int emit_stride,
                                                           const float *__restrict__ g_pts3d, EmitFrame F)
{
    RELOC_SMALL_KERNEL_PRIO();
    const int C = cur_count(F.n_cur_p, n_cur_max);
    db_ratio_emit_body<NW>(C, db, off, n_ids_max, ratio, min_rows, gate_off, emit_stride, g_pts3d, F);
}

// the same for up to 8 frames in one launch: blockIdx.y = frame
__global__ __launch_bounds__(256) void k_db_ratio_emit_batch(const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_ids_max,
                                                             int n_cur_max, double ratio, int min_rows, int gate_off, int emit_stride,
                                                             const float *__restrict__ g_pts3d, EmitBatch bt)
{
    RELOC_SMALL_KERNEL_PRIO();
    const EmitFrame &F = bt.f[blockIdx.y];
    const int C = cur_count(F.n_cur_p, n_cur_max);
    db_ratio_emit_body<4>(C, db, off, n_ids_max, ratio, min_rows, gate_off, emit_stride, g_pts3d, F);
}

// The emit pass under RELOC_MATCH_RATIO: launch_db_emit's arguments and shapes (8 waves for latency, 4 beside scans, the batch
// kernel for several frames) with the ratio and the record-length gate of the tick (min_rows, gate_off: db_ratio_emit_body).
// A list holds up to n_cur_max entries, so that many must fit the list stride.
int launch_db_ratio_emit(reloc_ctx *const *ctxs, int n, const EmitBatch &bt, const uint8_t *db_desc, const int64_t *db_off,
                         const float *g_pts3d, int n_ids_max, int n_cur_max, int emit_stride, double ratio, int min_rows, int gate_off,
                         bool latency)
{
    reloc_ctx *c0 = ctxs[0];
    if (n < 1 || n > RELOC_BATCH_MAX) { reloc_set_error("emit: 1..%d frames", RELOC_BATCH_MAX); return RELOC_E_ARG; }
    if (n_ids_max <= 0) return RELOC_OK;
    if (int rc = scan_capacity_check("db scan", n_cur_max)) return rc;
    if (n_cur_max > emit_stride) {
        reloc_set_error("ratio match lists: %d current descriptors do not fit the list stride of %d", n_cur_max, emit_stride);
        return RELOC_E_CAPACITY;
    }
    const int grid = n_ids_max < c0->num_cu * 16 ? n_ids_max : c0->num_cu * 16;
    const uint4 *desc = (const uint4 *)db_desc;
    if (n > 1)
        hipLaunchKernelGGL(k_db_ratio_emit_batch, dim3(grid, n), dim3(256), 0, c0->stream, desc, db_off, n_ids_max, n_cur_max, ratio,
                           min_rows, gate_off, emit_stride, g_pts3d, bt);
    else if (latency)
        hipLaunchKernelGGL(k_db_ratio_emit<8>, dim3(grid), dim3(512), 0, c0->stream, desc, db_off, n_ids_max, n_cur_max, ratio,
                           min_rows, gate_off, emit_stride, g_pts3d, bt.f[0]);
    else
        hipLaunchKernelGGL(k_db_ratio_emit<4>, dim3(grid), dim3(256), 0, c0->stream, desc, db_off, n_ids_max, n_cur_max, ratio,
                           min_rows, gate_off, emit_stride, g_pts3d, bt.f[0]);
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

// The whole-database scans of n contexts under RELOC_MATCH_RATIO (scan_counts): k_db_ratio with the tick's mask, stand-down and
// record-length gate for one frame, k_db_ratio_batch (blockIdx.y = frame) for several.  Records are dealt statically over
// one resident generation of workgroups, as reloc_db_ratio_counts deals them.
int launch_db_ratio_scan(reloc_ctx *const *ctxs, int n, const double *base_poses, double cos_tol, bool auto_mode)
{
    reloc_ctx *c0 = ctxs[0];
    if (n < 1 || n > RELOC_BATCH_MAX) { reloc_set_error("scan batch: 1..%d frames", RELOC_BATCH_MAX); return RELOC_E_ARG; }
    const DbArena &db = ctx_db(c0);
    const int n_ids = (int)db.records;
    if (n_ids <= 0) return RELOC_OK;
    if (int rc = scan_capacity_check("ratio scan", c0->max_feat)) return rc;
    const int grid = n_ids < c0->num_cu * 4 ? n_ids : c0->num_cu * 4;
    const uint4 *desc = (const uint4 *)db.desc;
    if (n == 1) {
        ScanMask mask;
        if (base_poses) {
            mask.xyh = db.xy_heading;
            for (int k = 0; k < 4; ++k) mask.q[k] = base_poses[3 + k];
        }
        mask.cos_tol = cos_tol;
        mask.skip_if = auto_mode ? c0->tick.cand_n : nullptr;
        hipLaunchKernelGGL(k_db_ratio<true>, dim3(grid), dim3(256), 0, c0->stream, desc, db.off, n_ids, (const uint4 *)c0->orb.buf.f_desc,
                           (const int32_t *)c0->orb.buf.f_count, c0->max_feat, c0->match.ratio, db.counts, mask, c0->prm.min_matches);
    } else {
        static const double identity[4] = {0.0, 0.0, 0.0, 1.0};
        const ScanBatch bt = scan_batch(ctxs, n, auto_mode, base_poses ? db.xy_heading : nullptr, cos_tol,
                                        [&](int g) { return base_poses ? base_poses + 7 * g + 3 : identity; });
        hipLaunchKernelGGL(k_db_ratio_batch, dim3(grid, n), dim3(256), 0, c0->stream, desc, db.off, n_ids, c0->max_feat, c0->match.ratio,
                           bt, c0->prm.min_matches);
    }
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

// ---------------------------------------------------------------------------------------------
// C-ABI entry points
// knnMatch(q, t, k=2) + Lowe test: t is the one record of a database of its own and q the current descriptors of the ratio
// emit pass, the way reloc_match_mutual runs the crossCheck one; nothing runs beside it: 8 waves
RELOC_API int reloc_match_ratio(reloc_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, double ratio, int32_t *qidx,
                                int32_t *tidx, int32_t *dist, int32_t *n_out)
{
    ARG_CHECK_CTX(ctx, n_out && nq >= 0 && nt >= 0, "reloc_match_ratio");
    *n_out = 0;
    ARG_CHECK(ratio - ratio == 0.0 && ratio > 0.0 && ratio <= 1.0, "reloc_match_ratio: ratio must be finite and in (0, 1]");
    if (nq == 0 || nt == 0) return RELOC_OK;
    ARG_CHECK(q && t && qidx && tidx && dist, "reloc_match_ratio: NULL array");
    if (nq > 65535) { reloc_set_error("ratio match: more than 65535 query descriptors"); return RELOC_E_CAPACITY; }
    if (nt >= (1 << RATIO_KEY_SHIFT)) { reloc_set_error("ratio match: train set too large"); return RELOC_E_CAPACITY; }
    return match_one_record(ctx, q, nq, 0, t, nt, false, qidx, tidx, dist, n_out, [&](const EmitBatch &bt, const uint8_t *rec, const int64_t *off) {
        return launch_db_ratio_emit(&ctx, 1, bt, rec, off, nullptr, 1, nq, nq, ratio, 0, 0, true);
    });
}

RELOC_API int reloc_db_ratio_counts(reloc_ctx *ctx, const uint8_t *cur, int n_cur, double ratio, int32_t *counts)
{
    ARG_CHECK_CTX(ctx, counts && n_cur >= 0 && (n_cur == 0 || cur) && ratio > 0, "reloc_db_ratio_counts");
    if (!db_ready(ctx)) { reloc_set_error("no database uploaded"); return RELOC_E_STATE; }
    const DbArena &db = ctx_db(ctx);
    if (n_cur == 0) { memset(counts, 0, (size_t)db.records * 4); return RELOC_OK; }
    if (int rc = scan_capacity_check("ratio scan", n_cur)) return rc;
    HostStaging st{ctx};
    const uint8_t *dc = st.upload_slot(0, cur, (int64_t)n_cur * 32);
    int grid = ctx->num_cu * 4;
    if (grid > db.records) grid = (int)db.records;
    st.launch(k_db_ratio<false>, dim3(grid), dim3(256), (const uint4 *)db.desc, db.off, (int)db.records, (const uint4 *)dc,
              (const int32_t *)nullptr, n_cur, ratio, db.counts, ScanMask{}, 0);
    st.download(counts, db.counts, db.records * 4);
    return st.finish();
}
