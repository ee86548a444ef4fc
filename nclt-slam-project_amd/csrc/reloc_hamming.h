// reloc_hamming.h -- what the four Hamming-matching files (reloc_scan.hip, reloc_scan_rows.hip, reloc_ratio.hip, reloc_match.hip)
// share and no other file includes: the distance and key primitives that more than one kernel family uses, the frame tables of
// the batched launches, the launchers that cross those files and the host staging of a single record.
//
// No MFMA: this is bitwise work.  Instruction costs measured on MI355X (tools/ubench_valu.hip,
// profiles/ubench_valu_r1.log): v_xor/v_or/v_and/v_add_u32 and the 16-bit v_min_u16 /
// v_lshlrev_b16 issue in ~2.5 cycles per wave64, while v_bcnt_u32_b32, 32-bit min/shift and every
// three-operand VOP3 (v_lshl_or, v_min3, v_add3...) take ~4.2.  The kernels are built around that:
//   - the accumulate form  v_bcnt_u32_b32 D, S0, S1 (D = popcount(S0) + S1)  keeps a 256-bit pair
//     at 8 xor + 8 bcnt (about 54 cycles per 64 pairs per SIMD: the floor of this problem);
//   - the argmin bookkeeping uses ONE 16-bit key per pair for both directions
//     (distance << 7 | row-in-chunk << 3 | column slot), built by one v_fmaak_f32 on the f32-denormal
//     bit patterns (see key_fma) and reduced with two v_min_u16, all in the cheap class.
#pragma once
#include <stdlib.h>
#include <type_traits>
#include <utility>

#include "reloc_internal.h"

typedef uint32_t u32;

__device__ __forceinline__ u32 bcnt_acc(u32 x, u32 acc)
{
    u32 r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}
__device__ __forceinline__ u32 min_u16(u32 a, u32 b)
{
    u32 r;
    asm("v_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ u32 max_u16(u32 a, u32 b)
{
    u32 r;
    asm("v_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// The scan's argmin key d << 7 | idx in ONE full-rate instruction: d < 2^9 and the key < 2^16, so read as f32 bit patterns
// d, idx and the key are positive denormals (x * 2^-149) and d * 128.0f + idx is exact -- the result's bit pattern IS the
// integer key.  Needs f32 denormals kept (.amdhsa_float_denorm_mode_32 3, the default without fast-math; guarded by
// tests/test_scan_denormals.py): flushed, every key would be 0.  c128 = 128.0f in a VGPR (v_fmaak_f32's multiplicand must
// be one); idx is the literal.
template <u32 IDX>
__device__ __forceinline__ u32 key_fma(u32 d, u32 c128)
{
    u32 r;
    asm("v_fmaak_f32 %0, %1, %2, %3" : "=v"(r) : "v"(d), "v"(c128), "n"(IDX));
    return r;
}
__device__ __forceinline__ u32 ham8(const u32 q[8], const uint4 a, const uint4 b, u32 init)
{
    u32 acc = init;
    acc = bcnt_acc(q[0] ^ a.x, acc);
    acc = bcnt_acc(q[1] ^ a.y, acc);
    acc = bcnt_acc(q[2] ^ a.z, acc);
    acc = bcnt_acc(q[3] ^ a.w, acc);
    acc = bcnt_acc(q[4] ^ b.x, acc);
    acc = bcnt_acc(q[5] ^ b.y, acc);
    acc = bcnt_acc(q[6] ^ b.z, acc);
    acc = bcnt_acc(q[7] ^ b.w, acc);
    return acc;
}

// two independent 256-bit distances with their instruction chains interleaved: an in-order wave
// then always has an independent instruction behind a v_bcnt (SQ_WAIT_INST_ANY was 40 % of wave time
// with one serial xor -> bcnt chain per pair at 4 waves per SIMD)
__device__ __forceinline__ void ham8x2(const u32 q0[8], const u32 q1[8], const uint4 a, const uint4 b, u32 init0, u32 init1,
                                       u32 &d0, u32 &d1)
{
    const u32 w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    u32 acc0 = init0, acc1 = init1;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const u32 x0 = q0[k] ^ w[k], x1 = q1[k] ^ w[k];
        acc0 = bcnt_acc(x0, acc0);
        acc1 = bcnt_acc(x1, acc1);
    }
    d0 = acc0;
    d1 = acc1;
}

// NC 256-bit distances of one row (8 wave-uniform words w, SGPRs) against NC descriptors held in registers, as NC
// accumulator chains visited round-robin, word by word: xor, its v_bcnt, next column.  The order is pinned with
// asm volatile because it is the whole point -- measured on MI355X (tools/exp_matrix2.hip, 20000 x 20000, same run):
//   2 chains interleaved (accumulator reused after 4 instructions)      190 us  2.10 T pairs/s   (compiler-scheduled: same)
//   4 chains                                                          187 us
//   8 chains, xor directly followed by its own v_bcnt                   160 us  2.49 T pairs/s
//   8 chains, xor issued one step ahead of its v_bcnt                   189 us
//   16 chains                                                           same as 8
// i.e. a v_bcnt must not read the accumulator a v_bcnt wrote fewer than ~16 instructions earlier, while the xor -> bcnt
// pair itself wants to stay adjacent.  The compiler's scheduler, left free with the same 8 accumulators, produces 187 us.
// One statement per INSTRUCTION on purpose: the compiler then puts an `s_nop 0` between each xor and its bcnt (61 per
// row), and that spacing is part of the result -- the same order written as one asm block per word, same run, whole
// matrix kernel: xor; bcnt back to back 202 us, xor; s_nop 0; bcnt 188, xor; bcnt; s_nop 0 186, this form 177
// (profiles/r2_exp_matrix2_spacing.log); in k_db_scan the block form without the s_nop costs 170.7 vs 161.0 us.
template <int NC>
__device__ __forceinline__ void ham8_cols(const u32 (&q)[NC][8], const u32 (&w)[8], u32 (&h)[NC])
{
    // the first word starts each accumulator from the inline constant 0 (no v_mov per chain and row: 158.7 -> 156.3 us)
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            u32 x;
            asm volatile("v_xor_b32 %0, %1, %2" : "=v"(x) : "s"(w[k]), "v"(q[j][k]));
            if (k == 0) asm volatile("v_bcnt_u32_b32 %0, %1, 0" : "=v"(h[j]) : "v"(x));
            else asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(h[j]) : "v"(x));
        }
}

// ---- scalar-cache row prefetch ------------------------------------------------------------------
// A teach row (32 B, wave-uniform address) arrives through the scalar cache.  Left alone, the compiler
// places each scalar load directly in front of its first use, which stalls the wave for the whole
// scalar-cache latency once per row.  scan_chunk instead issues the fetch of row t+1 between "row t has
// landed" and "row t is used": srow_landed() is an empty asm that reads one dword of row t, so the
// compiler's own waitcnt bookkeeping puts the wait for row t there (scalar loads return out of order:
// any wait is a wait for all of them, hence exactly one fetch in flight), and sched barriers keep the
// next fetch above the ~180 VALU instructions that hide its latency.
__device__ __forceinline__ void srow_landed(u32 first_dword) { asm volatile("" ::"s"(first_dword)); }

__device__ __forceinline__ u32 umin(u32 a, u32 b) { return a < b ? a : b; }
__device__ __forceinline__ double uniform_f64(double v)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ u32 umax(u32 a, u32 b) { return a > b ? a : b; }

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in order
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// the current descriptors of a launch: the count on the device when there is one, never more than the buffer's capacity
__device__ __forceinline__ int cur_count(const int32_t *n_cur_p, int n_cur_max) { return n_cur_p ? min(*n_cur_p, n_cur_max) : n_cur_max; }

// ---- frame tables of the batched launches ---------------------------------------------------------
// One frame of an emit pass (k_db_scan_emit*, k_db_ratio_emit*): the candidate records, the current descriptors, the match
// lists and the 3-D / 2-D pairs; EmitBatch: up to 8 of them in the kernel arguments, blockIdx.y = frame.
struct EmitFrame {
    const int32_t *rec_ids, *n_ids_p; const uint4 *cur; const int32_t *n_cur_p;
    int32_t *m_qidx, *m_tidx, *m_dist, *m_n; const float *g_xy; float *g_obj, *g_img;
};
struct EmitBatch { EmitFrame f[RELOC_BATCH_MAX]; };
// what the emit pass of a tick reads and writes of a context: its candidates against its features, match lists and pairs
static EmitFrame emit_frame(const reloc_ctx *c)
{
    EmitFrame F;
    const TickState &t = c->tick;
    const OrbFrame &o = c->orb.buf;
    F.rec_ids = t.cand_ids; F.n_ids_p = t.cand_n; F.cur = (const uint4 *)o.f_desc; F.n_cur_p = o.f_count;
    F.m_qidx = t.m_qidx; F.m_tidx = t.m_tidx; F.m_dist = t.m_dist; F.m_n = t.m_n; F.g_xy = o.f_xy; F.g_obj = t.p_obj; F.g_img = t.p_img;
    return F;
}

// Several frames in ONE launch (BASELINE.json config 4: batched relocalization): workgroup b scans frame b % B -- its
// current descriptors, feature count, counts array, heading and ticket counters -- so B whole-database scans share one
// launch: the launch-fixed cost (descriptor prologue per workgroup, last-record tail, kernel boundary) is paid once per
// batch, and the deal stays dynamic per frame.  Frames whose local search found candidates (AUTO mode) stand down alone.
struct ScanBatch {
    int n;
    const uint4 *cur[RELOC_BATCH_MAX];
    const int32_t *n_cur[RELOC_BATCH_MAX];
    int32_t *counts[RELOC_BATCH_MAX];
    const int32_t *skip_if[RELOC_BATCH_MAX];
    double q[RELOC_BATCH_MAX][4];
    const double *xyh;
    double cos_tol;
};
// frame f of a batched scan as the mask its body takes (db_count_body, db_ratio_body)
__device__ __forceinline__ ScanMask scan_mask_of(const ScanBatch &bt, int f)
{
    ScanMask mask;
    mask.xyh = bt.xyh;
    for (int k = 0; k < 4; ++k) mask.q[k] = bt.q[f][k];
    mask.cos_tol = bt.cos_tol;
    mask.skip_if = bt.skip_if[f];
    return mask;
}
// The table of n contexts' scans: frame f = ctxs[f]'s current features, counted into the counts of ctxs[f]'s arena.  xyh: the
// heading table of the database or NULL (no mask); quat(g): frame g's base_link quaternion x y z w; auto_mode: frames whose
// local search found candidates stand down on the device.
template <typename Quat>
static inline ScanBatch scan_batch(reloc_ctx *const *ctxs, int n, bool auto_mode, const double *xyh, double cos_tol, Quat quat)
{
    ScanBatch bt;
    bt.n = n;
    bt.xyh = xyh;
    bt.cos_tol = cos_tol;
    frame_slots(ctxs, n, [&](int f, reloc_ctx *c, int g) {
        bt.cur[f] = (const uint4 *)c->orb.buf.f_desc; bt.n_cur[f] = c->orb.buf.f_count; bt.counts[f] = ctx_db(c).counts;
        bt.skip_if[f] = auto_mode ? c->tick.cand_n : nullptr;
        const double *q = quat(g);
        for (int k = 0; k < 4; ++k) bt.q[f][k] = q[k];
    });
    return bt;
}

// ---- host side: what the launchers of the four files share ---------------------------------------
// The capacities a scan launcher checks before it launches: column indices are kept in 16 bits, a record's row keys in the
// LDS of one workgroup (max_rows 0: a launcher whose kernels keep no row keys).
static inline int scan_capacity_check(const char *who, int n_cur_max, int max_rows = 0)
{
    if (n_cur_max > 65535) { reloc_set_error("%s: more than 65535 current descriptors", who); return RELOC_E_CAPACITY; }
    if (max_rows > MAX_REC_ROWS) { reloc_set_error("%s: record larger than %d rows", who, MAX_REC_ROWS); return RELOC_E_CAPACITY; }
    return RELOC_OK;
}

// The launchers that cross the matching files.  launch_db_count_rows (reloc_scan_rows.hip): the few-query branch of
// launch_db_count, which keeps the condition that selects it -- no heading mask, at most 64 current descriptors, no record of
// more than SQ_MAX_ROWS rows; n_ids > 0 records of the database desc / off.  launch_db_ratio_emit (reloc_ratio.hip): the emit
// pass of launch_tick_emit under RELOC_MATCH_RATIO.
constexpr int SQ_MAX_ROWS = 1024;
int launch_db_count_rows(reloc_ctx *ctx, const uint4 *desc, const int64_t *off, int n_ids, const uint8_t *cur, const int32_t *n_cur_dev,
                         int n_cur_max, int32_t *counts);
int launch_db_ratio_emit(reloc_ctx *const *ctxs, int n, const EmitBatch &bt, const uint8_t *db_desc, const int64_t *db_off,
                         const float *g_pts3d, int n_ids_max, int n_cur_max, int emit_stride, double ratio, int min_rows, int gate_off,
                         bool latency);

// A single record as a database of its own, for the host-pointer matchers (reloc_match_mutual, reloc_match_ratio): q in slot 0
// (q_pad bytes behind it), t in slot 1; slot 2 holds the offsets {0, rows of the record}, the list length and three match lists
// of nq entries.  The record is q (rec_is_q) or t, the other side the current descriptors of frame 0.  launch(bt, record,
// offsets) enqueues the emit pass; the list length decides what comes back.
template <typename Launch>
static inline int match_one_record(reloc_ctx *ctx, const uint8_t *q, int nq, int q_pad, const uint8_t *t, int nt, bool rec_is_q,
                                   int32_t *qidx, int32_t *tidx, int32_t *dist, int32_t *n_out, Launch launch)
{
    HostStaging st{ctx};
    uint8_t *dq = st.slot<uint8_t>(0, (int64_t)nq * 32 + q_pad), *dt = st.slot<uint8_t>(1, (int64_t)nt * 32);
    int64_t *doff = (int64_t *)st.slot_bytes(2, (int64_t)nq * 12 + 64);
    if (st.rc) return st.rc;
    const int64_t offs[2] = {0, rec_is_q ? nq : nt};
    int32_t *dn = (int32_t *)(doff + 2);
    int32_t *dqi = dn + 4, *dti = dqi + nq, *ddi = dti + nq;
    st.upload(doff, offs, sizeof(offs));
    st.upload(dq, q, (int64_t)nq * 32);
    st.upload(dt, t, (int64_t)nt * 32);
    EmitBatch bt = {};
    bt.f[0].cur = (const uint4 *)(rec_is_q ? dt : dq); bt.f[0].m_qidx = dqi; bt.f[0].m_tidx = dti; bt.f[0].m_dist = ddi; bt.f[0].m_n = dn;
    st.run([&] { return launch(bt, rec_is_q ? dq : dt, doff); });
    const int32_t n = st.count(dn);
    if (n > 0) {
        st.download(qidx, dqi, (int64_t)n * 4);
        st.download(tidx, dti, (int64_t)n * 4);
        st.download(dist, ddi, (int64_t)n * 4);
    }
    if (int rc = st.finish()) return rc;
    *n_out = n;
    return RELOC_OK;
}
