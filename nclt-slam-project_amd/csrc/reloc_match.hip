// reloc_match.hip -- 256-bit Hamming matching on gfx950 (CDNA4), XOR + popcount on the VALU.
//
// Serves cv2.BFMatcher(NORM_HAMMING, crossCheck=True).match        (reference M:211,327; G:337)
//        cv2.BFMatcher(NORM_HAMMING, crossCheck=False).knnMatch k=2 (reference S:46,68)
//        the whole-database candidate scoring of variant G          (reference G:329-344)
//        knnMatch k=2 + Lowe test as the tick's match policy          (reference S:68-77; k_db_ratio*, k_db_ratio_emit*)
// and the all-pairs u16 distance matrix of BASELINE.json config 5.
// The file holds the kernels, their launchers and the entry points that scan (reloc_match_*, reloc_hamming_matrix*,
// reloc_db_match_counts*, reloc_db_ratio_counts, reloc_match_ratio); the database they scan is kept by reloc_db.hip.
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
// Hot kernel (k_db_scan): a wave keeps all 512 current-frame descriptors (8 per lane, 64 VGPRs);
// a database record's teach rows are wave-uniform, arrive through the scalar cache
// (s_load_dwordx8, the fetch of row t+1 issued as soon as row t has landed) and feed the VALU as
// SGPR operands, so one 32-byte scalar fetch pays for 512 pairs and no LDS traffic is in the
// inner loop.  A record's rows are dealt to the 4 waves of a workgroup as balanced contiguous
// ranges, walked in 16-row chunks and finished with ONE flexible chunk of 1-15 rows.  Per chunk a wave produces (a) per lane and column the best row
// (running 16-bit minimum), merged into LDS with ds_min_u32, and (b) per row the best column:
// an in-lane 8-way 16-bit minimum, then a register-tile butterfly across lanes
// (v_permlane16_swap / ds_bpermute).  Mutual nearest neighbours are resolved in LDS; k_db_scan
// leaves the per-record count, k_db_scan_emit the (queryIdx, trainIdx, distance) list in queryIdx
// order.  Keys are (distance << k | index): the minimum of packed keys is the smallest distance
// with the LOWEST index on ties, which is the tie rule of the specification.
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

// One butterfly exchange: on entry a = vector i, b = vector i+K on every lane.  On exit the
// return value on lane l is min over lanes {l, l^K} of (bit K of l ? vector i+K : vector i).
template <int K>
__device__ __forceinline__ u32 bfly(u32 a, u32 b, int lane)
{
    if constexpr (K == 32) {
        auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
        return umin(r[0], r[1]);
    } else if constexpr (K == 16) {
        auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
        return umin(r[0], r[1]);
    } else {
        const bool hi = lane & K;
        const u32 mine = hi ? b : a;
        const u32 theirs = hi ? a : b;
        return umin(mine, dpp_xor<K>(theirs));
    }
}

// The same exchange with the lane movement IN the minimum (v_min_u32 with a DPP operand) for the lane bits where a bank mask
// can tell the two halves apart: bit 2 (K = 4: row_shl:4 on banks 0 / 2 serves the lanes that keep vector a, row_shr:4 on banks
// 1 / 3 those that keep b -- a lane needs only ITS vector's partner) and bit 3 (K = 8: row_ror:8, banks 0-1 / 2-3).  Two
// instructions instead of two selects, a DPP move and a minimum.  Inline asm: the s_nop covers the two wait states a DPP read
// needs after a VALU write of its source, which the compiler does not count for an asm statement.
template <int K>
__device__ __forceinline__ u32 bfly_dpp(u32 a, u32 b)
{
    static_assert(K == 4 || K == 8, "bank-maskable lane bits only");
    u32 r;
    if constexpr (K == 4)
        asm("s_nop 1\n\tv_min_u32_dpp %0, %1, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
            "v_min_u32_dpp %0, %2, %2 row_shr:4 row_mask:0xf bank_mask:0xa" : "=&v"(r) : "v"(a), "v"(b));
    else
        asm("s_nop 1\n\tv_min_u32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_u32_dpp %0, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xc" : "=&v"(r) : "v"(a), "v"(b));
    return r;
}
// all-reduce over lane bit 0 / bit 1 (quad_perm exchange in the minimum)
__device__ __forceinline__ u32 allmin_quad(u32 x)
{
    asm("s_nop 1\n\tv_min_u32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "+v"(x));
    return x;
}

// ---- the two keys a chunk leaves in LDS, and what reads them back ---------------------------------
// A row's key enters the butterfly as best << 6 | lane, ONE v_lshl_or_b32 per row (the compiler splits the C form into a
// shift and an or: 32 instead of 16 instructions per chunk).  best = distance << 7 | row << 3 | slot, so the low nine bits
// of the result, slot << 6 | lane, ARE the column inside the wave's block and row_key() needs no field shuffle.
__device__ __forceinline__ u32 row_entry(u32 best, u32 lane)
{
    u32 v;
    asm("v_lshl_or_b32 %0, %1, 6, %2" : "=v"(v) : "v"(best), "v"(lane));
    return v;
}
// reduced row entry (distance << 13 | row << 9 | column in block) -> LDS row key, distance << 16 | column
__device__ __forceinline__ u32 row_key(u32 m, u32 colbase) { return ((m << 3) & 0xFFFF0000u) | ((m & 0x1FFu) | colbase); }
// 16-bit column minimum (distance << 7 | row in chunk << 3 | slot) -> LDS column key, distance << 16 | (tc + row in chunk).
// k16 << 9 has the distance in its upper half already; the lower half is REPLACED by tc + row in one SDWA add that writes
// bits 0-15 and keeps bits 16-31 (tc is wave-uniform and rides in the scalar operand; tc + row < 2^16 because the LDS keys
// hold a row in 16 bits): three instructions a column where shift, field, add and and-or took four.  The compiler does not
// count wait states for an asm statement: scan_chunk keeps every key's first reader NJ instructions behind this partial write.
__device__ __forceinline__ u32 col_key(u32 k16, int tc)
{
    u32 key = k16 << 9;
    const u32 row = (k16 >> 3) & 15u;
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:WORD_0 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD"
        : "+v"(key) : "s"(tc), "v"(row));
    return key;
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in order
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// One 16-row chunk of a record against the wave's 64*NJ columns; nr = the rows it really has (1..16).
//   q[j]    : descriptor of column colbase + j*64 + lane (padding columns repeat the last real column:
//             a duplicate offers the same distance with a larger index, so it never wins a minimum)
//   nr < 16 : the tail chunk of a wave's row range: the rows it does not have are skipped (wave-uniform branch) and enter the
//             butterfly as don't-cares, which only the unwritten lanes of those rows receive; their fetch addresses are
//             clamped to the record's last row
// One 16-bit key per pair serves both directions: distance << 7 | row-in-chunk << 3 | column slot.
// Among the rows of one column the slot bits are equal, so the minimum is (distance, row); among the
// columns of one row the row bits are equal, so the minimum is (distance, slot).  Per pair that is
// one v_fmaak_f32 (key_fma) + 2 v_min_u16 on top of the 16 instructions of the distance (through round 4: v_lshlrev_b16 +
// v_or_b32 for the key; the row's 8-way minimum with v_min3_f32 was measured and dropped, profiles/README.md
// "Dropped experiments" #9).
// The column minima leave the chunk in one of two forms (MERGE, a compile-time property of the CALLER):
//   MERGE_SHARED : converted to distance << 16 | (tc + row) (col_key) and merged with ds_min_u32 into the buffer all waves of
//                  the workgroup share -- the emit pass, and every record of the counting scan whose waves walk more than
//                  one chunk or column block;
//   MERGE_CHOICE : the counting scan.  n <= sliced_max (wave-uniform, per record) selects between the shared form and plain 16-bit
//                  stores of the raw minima into the calling wave's own slice (slice[j * 64 + lane]), which db_count_body
//                  resolves.  The choice is a scalar branch BEHIND the unrolled rows, never inside them, and not a second
//                  instantiation: the 16-row body is 45 KB of code and two of them in one kernel would not share the 64 KB
//                  instruction cache on a ragged database, where neighbouring workgroups take both paths.
enum ScanMerge { MERGE_SHARED, MERGE_CHOICE };
template <int NJ, ScanMerge MERGE = MERGE_SHARED>
__device__ __forceinline__ void scan_chunk(const uint4 *__restrict__ rec, int n, int tc, int nr, const u32 (&q)[NJ][8],
                                           u32 colbase, u32 *rowkey, u32 *colbest, bool single_cb, int lane,
                                           unsigned short *slice = nullptr, int sliced_max = -1)
{
    // (column minima in LDS instead of registers: measured and dropped, profiles/README.md "Dropped experiments" #1)
    u32 cb16[NJ];                                                      // seeded by row 0, which every chunk has (nr >= 1)
    const u32 c128 = 0x43000000u;                                      // 128.0f, key_fma's multiplicand
    // The 16 row keys are reduced by a register-tile butterfly, but AS THEY COME: the rows of the chunk
    // are visited in bit-reversed order (0, 8, 4, 12, ...), so the two operands of every butterfly node are
    // finished right after each other and at most log2(16) + 1 partial results are alive instead of 16 keys -- 11
    // VGPRs less, which takes the kernel from 115 to <= 104 registers: four resident workgroups then leave
    // 96 registers per SIMD lane free, enough for the small kernels of other streams to run BESIDE the scan.
    constexpr int R = 16, LOG_R = 4;
    u32 stk[LOG_R + 1];
    // Teach rows come through the scalar cache, one fetch in flight (see srow_landed).
    auto bitrev = [](int i) { int r = 0; for (int b = 0; b < LOG_R; ++b) r |= ((i >> b) & 1) << (LOG_R - 1 - b); return r; };
    auto row_of = [&](int i) { return min(tc + bitrev(i), n - 1); };   // wave-uniform
    uint4 a = rec[2 * row_of(0)], b = rec[2 * row_of(0) + 1];
    // compile-time row and column indices: the key constants are immediates.
    // (bookkeeping software-pipelined into the next row's chains: measured and dropped, profiles/README.md "Dropped experiments" #2)
    static_for<R>([&](auto ic_) {
        constexpr int i = decltype(ic_)::value;
        constexpr int t = [](int v) { int r = 0; for (int bb = 0; bb < LOG_R; ++bb) r |= ((v >> bb) & 1) << (LOG_R - 1 - bb); return r; }(i);
        srow_landed(a.x);                                                // this row is here ...
        uint4 na, nb;
        if (i + 1 < R) { na = rec[2 * row_of(i + 1)]; nb = rec[2 * row_of(i + 1) + 1]; }   // ... the next one on its way
        __builtin_amdgcn_sched_barrier(0);
        // A row the chunk does not have needs no key at all: the butterfly transposes, a lane's result is the minimum over lanes
        // of ITS row only, and the lanes of a missing row are not written below (row_in_chunk < nr).  So v is left undefined on
        // the skipped side -- an empty asm output, no instruction and no block.  (An `= 0xFFFFFFFF` default is set by the compiler
        // in front of the row's branch, one v_mov on the way of every row that IS there; pinned to the far side of the branch
        // it costs fifteen out-of-line blocks and 1 %: profiles/README.md "Dropped experiments" #10.)
        u32 v;
        asm("" : "=v"(v));
        if (t == 0 || t < nr) {                                          // wave-uniform
            u32 best = 0;
            const u32 w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            u32 h[NJ];
            ham8_cols<NJ>(q, w, h);                                    // NJ accumulator chains, order pinned
            static_for<NJ / 2>([&](auto jc_) {
                constexpr int j = 2 * decltype(jc_)::value;
                const u32 k0 = key_fma<t * 8 + j>(h[j], c128), k1 = key_fma<t * 8 + j + 1>(h[j + 1], c128);
                cb16[j] = t == 0 ? k0 : min_u16(cb16[j], k0);          // best row of column j
                cb16[j + 1] = t == 0 ? k1 : min_u16(cb16[j + 1], k1);
                best = j == 0 ? min_u16(k0, k1) : min_u16(best, min_u16(k0, k1));   // best column of this row
            });
            v = row_entry(best, (u32)lane);
        }
        // Node of level k joins rows t and t + 16 / 2^(k+1).  The four levels split on lane bits 2, 3 (DPP minima, two instructions
        // a node: the levels with 8 and 4 nodes), 4 and 5 (permlane swap + minimum), and the two lane bits left over are reduced
        // on the one value at the end: 32 instead of ~66 instructions per chunk and no select masks to keep (rounds 1-3: levels on
        // bits 3, 2, 1, 0 with select nodes -- two v_cndmask, a DPP move and a minimum each).  4-stream run +1.8 % (6 836 -> 6 958
        // frames/s, interleaved), and the kernel fits its 104 registers without scratch.  Lane l ends with row 8 b2 + 4 b3 + 2 b4 + b5.
        if constexpr ((i & 1) == 0) stk[0] = v;
        else {
            v = bfly_dpp<4>(stk[0], v);
            if constexpr ((i & 2) == 0) stk[1] = v;
            else {
                v = bfly_dpp<8>(stk[1], v);
                if constexpr ((i & 4) == 0) stk[2] = v;
                else {
                    v = bfly<16>(stk[2], v, lane);
                    if constexpr ((i & 8) == 0) stk[3] = v;
                    else stk[4] = bfly<32>(stk[3], v, lane);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (i + 1 < R) { a = na; b = nb; }
    });
    // lane bits 0, 1: every lane now holds the minimum of ITS row; one lane per row writes
    const u32 m = allmin_quad(stk[LOG_R]);
    const int row_in_chunk = ((lane >> 2) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 4) & 1) * 2 + (lane >> 5);
    const bool writer = (lane & 3) == 0;
    const int row = tc + row_in_chunk;
    if (writer && row_in_chunk < nr) {
        if (single_cb) rowkey[row] = row_key(m, 0);                  // one column block: colbase == 0
        else atomicMin(&rowkey[row], row_key(m, colbase));
    }
    if constexpr (MERGE == MERGE_CHOICE) {
        if (n <= sliced_max) {                                           // wave-uniform, one scalar compare
            // eight ds_write_b16, no VALU: lanes l and l + 1 share a dword, a 2-way store conflict costs no LDS cycle
#pragma unroll
            for (int j = 0; j < NJ; ++j) slice[j * 64 + lane] = (unsigned short)cb16[j];
            return;
        }
    }
    // all the column keys, then all the minima: a key's partial write is NJ instructions old before LDS reads the register
    u32 ck[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) ck[j] = col_key(cb16[j], tc);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) atomicMin(&colbest[colbase + j * 64 + lane], ck[j]);
}

// ---- what the counting scan and the emit pass share ---------------------------------------------
// NJ = columns per lane.  A wave covers a "column block" of 64*NJ current descriptors, kept in registers (load_q).
// NJ = 8 is the working point (500 descriptors are one block, 64 VGPRs of descriptors, 4 waves per SIMD);
// NJ = 4 / 2 serve calls with at most 256 / 128 current descriptors, see k_db_scan.  (8 waves per SIMD -- NJ = 4 with two blocks,
// or the descriptors in LDS -- measured slower: profiles/README.md "Dropped experiments" #3.)
// When the number of column blocks ncb divides the NW waves of a workgroup, wave w is bound to block w % ncb for the whole
// launch (its descriptors stay in registers) and shares a record's rows with the other waves bound to that block; otherwise
// every wave walks all column blocks and reloads its registers per block.
struct WaveBinding {
    bool bound;               // static wave -> column block binding
    int my_cb;                // the bound wave's column block
    int chunk0, chunk_step;   // this wave's place among, and the number of, the waves that share a block's rows
};
template <int NW>
__device__ __forceinline__ WaveBinding bind_wave(int wave, int ncb)
{
    const bool bound = (NW % ncb) == 0;
    return {bound, bound ? wave % ncb : 0, bound ? wave / ncb : wave, bound ? NW / ncb : NW};
}

// The emit pass: the match lists (queryIdx, trainIdx, distance, in queryIdx order) of a few records, dealt statically
// (record it = blockIdx.x, + gridDim.x, ...).  Dynamic LDS: (ncb*64*NJ + max_rows + 16) * 4 bytes.
// Record it of the launch is rec_ids[it] (rec_ids == NULL: it) and lists emit_stride entries apart; with g_obj set every
// mutual match also leaves its 3-D / 2-D pair (keypoints_3d_cam[queryIdx], pts_curr_2d[trainIdx], M:333-336) next to its
// index triplet, so no gather launch follows.
template <int NJ, int NW>
__device__ __forceinline__ void db_emit_body(
    u32 *lds, int C, const uint4 *__restrict__ db, const int64_t *__restrict__ off, const int32_t *__restrict__ rec_ids,
    const int32_t *__restrict__ n_ids_p, int n_ids_max, const uint4 *__restrict__ cur, int max_rows,
    int32_t *__restrict__ m_qidx, int32_t *__restrict__ m_tidx, int32_t *__restrict__ m_dist, int32_t *__restrict__ m_n,
    int emit_stride, const float *__restrict__ g_pts3d, const float *__restrict__ g_xy, float *__restrict__ g_obj,
    float *__restrict__ g_img)
{
    constexpr int CB = 64 * NJ;           // columns per block
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: row fetches stay scalar
    const int n_ids = n_ids_p ? min(*n_ids_p, n_ids_max) : n_ids_max;
    const int ncb = max((C + CB - 1) / CB, 1);
    u32 *colbest = lds;                   // ncb * CB : best (distance << 16 | row) per column
    u32 *rowkey = colbest + ncb * CB;     // max_rows : best (distance << 16 | column) per row
    u32 *wsum = rowkey + max_rows;        // 16       : mutual pairs per wave
    static_assert(NW == 1 || NW == 2 || NW == 4 || NW == 8, "wsum holds one word per wave");

    u32 q[NJ][8];
    auto load_q = [&](int colbase) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = min(colbase + j * 64 + lane, max(C - 1, 0));   // padding repeats the last column
            const uint4 a = cur[2 * col], b = cur[2 * col + 1];
            q[j][0] = a.x; q[j][1] = a.y; q[j][2] = a.z; q[j][3] = a.w;
            q[j][4] = b.x; q[j][5] = b.y; q[j][6] = b.z; q[j][7] = b.w;
        }
    };
    const WaveBinding wb = bind_wave<NW>(wave, ncb);
    if (wb.bound) load_q(wb.my_cb * CB);
    for (int it = blockIdx.x; it < n_ids; it += gridDim.x) {
        const int r = rec_ids ? rec_ids[it] : it;
        const int64_t row0 = off[r];
        const int n = (int)(off[r + 1] - row0);
        const uint4 *rec = db + 2 * row0;
        for (int i = tid; i < ncb * CB; i += 64 * NW) colbest[i] = 0xFFFFFFFFu;
        for (int i = tid; i < n; i += 64 * NW) rowkey[i] = 0xFFFFFFFFu;
        __syncthreads();
        if (n > 0 && C > 0) {
            for (int cb = wb.bound ? wb.my_cb : 0; cb < (wb.bound ? wb.my_cb + 1 : ncb); ++cb) {
                if (!wb.bound) load_q(cb * CB);
                // The record's rows are dealt to the waves bound to this column block as contiguous ranges, balanced to
                // the single row; a wave walks its range in 16-row chunks and finishes it with ONE flexible chunk of
                // 1-15 rows (n = 64, 4 waves: one 16-row chunk each; n = 45: 12/11/11/11 rows = one flexible chunk each
                // -- round 2 walked tails in 4-row chunks and paid the chunk epilogue, butterfly + 9 LDS minima, every 4
                // rows: 1.56 T pairs/s on 45-row records against 2.0 T on 64-row ones).
                const int per = n / wb.chunk_step, extra = n % wb.chunk_step;
                int tc = wb.chunk0 * per + min(wb.chunk0, extra);
                const int tend = tc + per + (wb.chunk0 < extra ? 1 : 0);
                // ONE instantiation serves full and partial chunks: the unrolled 16-row body is 45 KB of code, two of them
                // would not share the 64 KB instruction cache
#pragma nounroll
                for (; tc < tend; tc += 16)
                    scan_chunk<NJ>(rec, n, tc, min(16, tend - tc), q, (u32)(cb * CB), rowkey, colbest, ncb == 1, lane);
            }
        }
        __syncthreads();
        // mutual resolution, in teach-row (queryIdx) order
        u32 base = 0;
        for (int rb = 0; rb < n; rb += 64 * NW) {
            const int row = rb + tid;
            bool mutual = false;
            u32 key = 0;
            if (row < n && C > 0) {
                key = rowkey[row];
                const u32 col = key & 0xFFFFu;
                mutual = (colbest[col] & 0xFFFFu) == (u32)row;
            }
            const unsigned long long bal = __ballot(mutual);
            if (lane == 0) wsum[wave] = (u32)__popcll(bal);
            __syncthreads();
            u32 before = base;
            for (int w = 0; w < wave; ++w) before += wsum[w];
            u32 total = 0;
            for (int w = 0; w < NW; ++w) total += wsum[w];
            if (mutual) {
                const u32 pos = before + (u32)__popcll(bal & ((1ull << lane) - 1ull));
                const int64_t o = (int64_t)it * emit_stride + pos;
                m_qidx[o] = row;
                m_tidx[o] = (int32_t)(key & 0xFFFFu);
                m_dist[o] = (int32_t)(key >> 16);
                if (g_obj) {
                    const float *p3 = g_pts3d + 3 * (row0 + row), *p2 = g_xy + 2 * (size_t)(key & 0xFFFFu);
                    float *po = g_obj + 3 * o, *pi = g_img + 2 * o;
                    po[0] = p3[0]; po[1] = p3[1]; po[2] = p3[2];
                    pi[0] = p2[0]; pi[1] = p2[1];
                }
            }
            base += total;
            __syncthreads();
        }
        if (tid == 0 && m_n) m_n[it] = (int32_t)base;
    }
}

// The counting scan (no match lists) of the whole database.  grid: any; block: 256 (4 waves).  Dynamic LDS:
// (col_words + max_rows + 16) * 4 + 4 * 64 * NJ * 2 bytes (CountPlan).  mask.xyh != NULL: heading-incompatible records are not scored (count 0), see ScanMask.
// The per-record flow of db_emit_body reduced to TWO barriers per record:
//   - colbest is double-buffered: the buffer of the NEXT record is cleared while this record's chunks run, so no
//     clear / barrier pair stands in front of a record;
//   - with one column block (<= 64 * NJ current descriptors: every fused tick) each row key is written by exactly one
//     wave with a plain store and never needs clearing;
//   - with one column block and records of at most 64 rows (one chunk per wave) the column minima take the same road: raw
//     16-bit keys in a slice per wave, plain stores, resolved for the one column a row points at (`sliced` below);
//   - the mutual pairs are only counted: per wave one ballot and one LDS add, no prefix sums;
//   - the next record's ticket (drawn a record ahead) is settled between the same two barriers.
// A workgroup's FIRST record is dealt statically (record = workgroup index, no counter round trip in front of the first
// row); the counters deal the records behind the grid.  Round 2's flow had six barriers per record and waited for an
// atomic before the first row: 10 000 x 64 in three generations 162 -> [see DESIGN.md] us.
// The ticket counters of a launch, one per 128-byte line: per frame (<= RELOC_BATCH_MAX) the 8 per-XCD record counters, then
// one exit counter behind the last frame's; scan_alloc takes the largest pool a launch can use.
constexpr int TICKET_STRIDE = 32;
constexpr int SCAN_TICKET_WORDS = (RELOC_BATCH_MAX * 8 + 1) * TICKET_STRIDE;
template <int NJ>
__device__ __forceinline__ void db_count_body(
    u32 *lds, int C, const uint4 *__restrict__ db, const int64_t *__restrict__ off, const int32_t *__restrict__ rec_ids,
    const int32_t *__restrict__ n_ids_p, int n_ids_max, const uint4 *__restrict__ cur, int max_rows,
    int32_t *__restrict__ counts, const ScanMask &mask, u32 *ticket, int quota, int n_bounded, int col_words,
    u32 *ticket_pool = nullptr, int pool_frames = 1, int block = -1, int n_blocks = -1)
{
    // quota / n_bounded: the first n_bounded workgroups of a scan leave once they have served `quota` ROWS (their slots go to
    // whatever waits: with several contexts on the chip another stream's ORB / PnP kernel); their budgets add up to the whole
    // database, so they normally serve every record.  The eight workgroups behind them (one per XCD, the last to start) draw
    // until the counters run dry: whatever the budgets left over is served (nothing, when the host knew the row total).
    // (The variants dropped on the way, a quota of records among them: profiles/README.md "Dropped experiments" #4.)
    // ticket: the 8 per-XCD record counters of THIS scan; ticket_pool / pool_frames: all counters of the launch (a batched
    // launch scans pool_frames frames, frame f owning ticket_pool + f * 8 * TICKET_STRIDE; the word behind them counts
    // the workgroups that have left).  block / n_blocks: this workgroup's index and the number of workgroups of ITS scan
    // (default = the launch's).
    if (!ticket_pool) ticket_pool = ticket;
    if (block < 0) { block = blockIdx.x; n_blocks = gridDim.x; }
    constexpr int CB = 64 * NJ, NW = 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_ids = n_ids_p ? min(*n_ids_p, n_ids_max) : n_ids_max;
    const int ncb = max((C + CB - 1) / CB, 1);
    // col_words words of column minima (best distance << 16 | row per column), sized by the host from the CAPACITY of the
    // current-descriptor buffer (one buffer's worth, at least two column blocks); the kernel knows the COUNT: when two buffers
    // of ncb blocks fit they are double-buffered (the next record's buffer is cleared while this record's chunks run: two
    // barriers per record), otherwise one buffer is cleared between the records (three barriers).  A tick's ~500 features in
    // a context made for 8192 are one block: double-buffered in 33 KB, where sizing two buffers for the capacity took 66 KB
    // and left room for two workgroups per CU instead of four.
    const bool dbl = 2 * ncb * CB <= col_words;                                // workgroup-uniform
    u32 *colbuf = lds;
    u32 *rowkey = colbuf + col_words;         // max_rows     : best (distance << 16 | column) per row
    u32 *wsum = rowkey + max_rows;            // [0], [1]: mutual-pair counters of the two buffers; [8]: next record
    // Per-wave slices of raw column minima (NW x CB 16-bit keys, distance << 7 | row in chunk << 3 | slot), an LDS region of
    // their own, for the records in which no wave walks more than one chunk of one column block (`sliced` below): one column
    // block (every fused tick) and at most 16 rows per wave, i.e. records of up to 64 rows.  A wave then stores its minima
    // with plain stores (scan_chunk, MERGE_CHOICE) and the resolving wave rebuilds distance << 16 | absolute row for the ONE
    // column each row points at -- where the shared form converts all CB columns in every wave, merges them with ds_min_u32
    // and clears a buffer per record.  No atomics, no second buffer, no clear: a wave with rows overwrites its whole slice
    // in every such record, and the slice of a wave without rows is not read.
    unsigned short *slices = (unsigned short *)(wsum + 16);

    u32 q[NJ][8];
    auto load_q = [&](int colbase) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = min(colbase + j * 64 + lane, max(C - 1, 0));   // padding repeats the last column
            const uint4 a = cur[2 * col], b = cur[2 * col + 1];
            q[j][0] = a.x; q[j][1] = a.y; q[j][2] = a.z; q[j][3] = a.w;
            q[j][4] = b.x; q[j][5] = b.y; q[j][6] = b.z; q[j][7] = b.w;
        }
    };
    const WaveBinding wb = bind_wave<NW>(wave, ncb);
    // RELOC_TICK_AUTO: this scan stands down (scan-uniform).  Its workgroups still check out at the end, so that the last
    // workgroup of the launch can put the counters back
    const bool stand_down = mask.skip_if && *mask.skip_if != 0;
    if (wb.bound && !stand_down) load_q(wb.my_cb * CB);
    double hc = 1.0, hs = 0.0, cos_tol = 0.0;
    if (mask.xyh) {
        cur_heading_q(mask.q, hc, hs);
        cos_tol = mask.cos_tol;
        // wave-uniform values computed on the vector unit: moved to scalar registers (they live across the whole launch, and
        // the kernel is capped at 104 vector registers)
        hc = uniform_f64(hc); hs = uniform_f64(hs); cos_tol = uniform_f64(cos_tol);
    }
    // Work distribution.  ticket == NULL: record it = block, + n_blocks, ... (static).  Otherwise the grid is one
    // resident generation and every workgroup draws records from counters, so that all CUs stay full until the last
    // record (with a static deal the workgroups of a CU finish one after the other and the CU's tail runs at 3, 2, 1
    // waves per SIMD).  One counter serves ~88 draws per microsecond (measured: 10 000 draws on one word = 143 us), so
    // there are 8, one per XCD (HW_REG_XCC_ID) on its own 128-byte line; a workgroup whose counter has run dry moves on to
    // the next one.  The draw for the next record is in flight while the current one is processed.  The last workgroup to
    // leave zeroes all words.
    int shard = 0, dry = 0;
    if (ticket) {
        u32 x;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x));
        shard = (int)(x & 7u);
    }
    auto draw = [&]() -> u32 { return atomicAdd(&ticket[shard * TICKET_STRIDE], 1u); };
    // the dealing thread (`dealer` below): ticket -> record index; counter x deals records n_blocks + x, n_blocks + x + 8, ... (the first n_blocks
    // records are the workgroups' static first records)
    auto settle = [&](u32 t) -> int {
        for (;;) {
            const long long rec_i = (long long)n_blocks + (long long)shard + 8ll * (long long)t;
            if (rec_i < n_ids) return (int)rec_i;
            if (++dry >= 8) return n_ids;
            shard = (shard + 1) & 7;
            t = draw();
        }
    };
    int it = stand_down ? n_ids : block;
    int left = (quota > 0 && block < n_bounded) ? quota : 0x7fffffff;        // rows this workgroup may still take on
    // Per-record work goes to the wave that owns it, behind wave-uniform branches, so that the other waves walk to the barrier
    // and issue nothing: wave 0 counts the mutual pairs of rows 0-63 (wave w those of rows 64 w ...) and writes the count;
    // the last wave, the one the row deal gives the fewest rows, draws and settles the tickets in its first lane.
    const bool dealer = tid == 64 * (NW - 1);
    const int buf_words = ncb * CB;                                          // one buffer of column minima, a multiple of 128
    for (int i = tid; i < buf_words; i += 64 * NW) colbuf[i] = 0xFFFFFFFFu;
    if (tid == 0) wsum[0] = wsum[1] = 0;
    __syncthreads();
    int p = 0;
    const int sliced_max = ncb == 1 ? 16 * NW : -1;                          // most rows of a record that takes the slices
    while (it < n_ids) {
        u32 *colbest = colbuf + (dbl ? p * buf_words : 0);
        const int r = rec_ids ? rec_ids[it] : it;
        const bool scored = !(mask.xyh && !heading_ok(mask.xyh + 4 * (int64_t)r, hc, hs, cos_tol));      // workgroup-uniform
        const int64_t row0 = off[r];
        const int n_rec = scored ? (int)(off[r + 1] - row0) : 0;
        const int n = C > 0 ? n_rec : 0;                                 // rows to scan and to resolve: none without a column
        const uint4 *rec = db + 2 * row0;
        left -= max(n_rec, 1);
        u32 next_ticket = 0;
        if (ticket && dealer && left > 0) next_ticket = draw();          // no draw that this workgroup would not serve
        // Workgroup-uniform, per record: the column minima go through the per-wave slices (one column block, so the NW waves
        // share the rows and chunk_step == NW; at most one chunk per wave).  Ragged databases mix both forms record by record.
        // The shared buffer's invariant -- the buffer a record merges into (p when double-buffered, else the only one) holds
        // 0xFFFFFFFF in all its ncb * CB words when the record starts -- holds whichever form the record before took:
        //   - it holds for the first record (cleared in front of the loop);
        //   - a record in the shared form dirties buffer p only and leaves the next record's buffer clear, as before: p ^ 1,
        //     cleared beside its chunks and made current behind it, or the one buffer, cleared behind it;
        //   - a sliced record neither reads nor writes the shared buffers and leaves p alone, so the buffer that was clear
        //     when it started is the next record's buffer and still clear.  It therefore needs neither the clear nor the flip.
        // (One column block always fits twice: col_words >= 2 * CB.  The single-buffer regime has no sliced records at all.)
        // The counter wsum[p] of a sliced record is the one the record before may have used: thread 0 zeroes it behind that
        // record's last barrier, and the first add of this record comes behind this record's first barrier.
        // Tested where it is needed as ONE scalar compare of n against sliced_max (16 * NW with one column block, else -1; set
        // in front of the loop), each time on a copy of n the compiler cannot see through: kept as one flag across the
        // chunk it becomes a 64-bit lane mask that is spilled to and read back from VGPR lanes in every wave and record.
        auto sliced = [&]() { int nn = n; asm volatile("" : "+s"(nn)); return nn <= sliced_max; };
        if (n > 0) {
            if (ncb > 1) {                                               // several waves write one row's key: atomic minima
                for (int i = tid; i < n; i += 64 * NW) rowkey[i] = 0xFFFFFFFFu;
                __syncthreads();
            }
            // the row walk and load_q are db_emit_body's, written out again: as shared functions they perturb this kernel's code
            for (int cb = wb.bound ? wb.my_cb : 0; cb < (wb.bound ? wb.my_cb + 1 : ncb); ++cb) {
                if (!wb.bound) load_q(cb * CB);
                const int per = n / wb.chunk_step, extra = n % wb.chunk_step;
                int tc = wb.chunk0 * per + min(wb.chunk0, extra);
                const int tend = tc + per + (wb.chunk0 < extra ? 1 : 0);
#pragma nounroll
                for (; tc < tend; tc += 16)
                    scan_chunk<NJ, MERGE_CHOICE>(rec, n, tc, min(16, tend - tc), q, (u32)(cb * CB), rowkey, colbest, ncb == 1, lane,
                                                 slices + wave * CB, sliced_max);
            }
        }
        if (!sliced()) {
            asm volatile("");   // keeps the two tests apart: merged, every sliced record reads dbl's spilled lane mask back
            if (dbl) {   // the other buffer, for the next record: two words a lane, 128 a wave and step (512 words: one store each)
                u32 *other = colbuf + (p ^ 1) * buf_words;
                for (int base = 0; base + 128 * wave < buf_words; base += 128 * NW) {  // wave-uniform
                    other[base + 2 * tid] = 0xFFFFFFFFu;
                    other[base + 2 * tid + 1] = 0xFFFFFFFFu;
                }
            }
        }
        __syncthreads();                                                  // every minimum of this record is in LDS
        if (sliced()) {
            // At most 64 rows: wave 0 resolves them all (64 * wave < n, the shared form's own wave-uniform test).  Row `tid`
            // points at column col; of that column every wave that had rows (wave w has some iff w < n: the deal gives
            // n / NW rows and the first n % NW waves one more) left its best (distance, row in chunk).
            // distance << 16 | (tc_w + row in chunk), tc_w from that deal, is the key the wave would have merged with
            // ds_min_u32, and the minimum over the waves is what the shared buffer would hold: the smallest distance, on
            // ties the lowest absolute row.
            if (64 * wave < n) {
                asm volatile("");   // a scalar branch for the waves without rows, not folded into the lane test below
                if (tid < n) {
                    const u32 col = rowkey[tid] & 0xFFFFu;
                    const int per = n / NW, extra = n % NW;
                    u32 best = 0xFFFFFFFFu;
#pragma unroll
                    for (int w = 0; w < NW; ++w)
                        if (w < n) {                                      // wave-uniform
                            const u32 k = slices[w * CB + col];
                            const u32 tc_w = (u32)(w * per + min(w, extra));
                            best = umin(best, ((k << 9) & 0xFFFF0000u) | (tc_w + ((k >> 3) & 15u)));
                        }
                    const unsigned long long mutual = __builtin_amdgcn_ballot_w64((best & 0xFFFFu) == (u32)tid);
                    if (lane == 0 && mutual) atomicAdd(&wsum[p], (u32)__popcll(mutual));
                }
            }
        } else
        for (int rb = 0; rb + 64 * wave < n; rb += 64 * NW) {             // wave-uniform: a wave without rows goes on to the barrier
            const int row = rb + tid;
            if (row < n) {                                                // the wave's first lane always is
                const u32 col = rowkey[row] & 0xFFFFu;
                const unsigned long long mutual = __builtin_amdgcn_ballot_w64((colbest[col] & 0xFFFFu) == (u32)row);
                if (lane == 0 && mutual) atomicAdd(&wsum[p], (u32)__popcll(mutual));
            }
        }
        if (dealer) wsum[8] = ticket ? (left > 0 ? (u32)settle(next_ticket) : (u32)n_ids) : (u32)(it + n_blocks);
        __syncthreads();
        if (tid == 0) {
            counts[r] = (int32_t)wsum[p];
            wsum[p] = 0;
        }
        it = __builtin_amdgcn_readfirstlane((int)wsum[8]);
        if (sliced()) continue;                                           // shared buffers untouched: nothing to flip or clear
        if (dbl) p ^= 1;
        else {       // one buffer: cleared between the records
            for (int i = tid; i < ncb * CB; i += 64 * NW) colbuf[i] = 0xFFFFFFFFu;
            __syncthreads();
        }
    }
    if (ticket && tid == 0) {
        const int words = pool_frames * 8;
        if (atomicAdd(&ticket_pool[words * TICKET_STRIDE], 1u) == gridDim.x - 1) {      // every other workgroup has made its last draw
            for (int x = 0; x <= words; ++x)
                __hip_atomic_store(&ticket_pool[x * TICKET_STRIDE], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The kernels proper.  NJ is chosen by the host from the CAPACITY of the current-descriptor buffer: entry points
// that know the query count (reloc_db_match_counts*, reloc_match_mutual) scan 128 or 256 columns per wave when
// that is enough, so their cost follows the query count instead of being flat below 512; the fused tick passes
// its feature capacity and always runs NJ = 8.  (One kernel branching on the device-side count was measured:
// it costs the NJ = 8 path 3 %.)
template <int NJ>
__global__ __launch_bounds__(256, 4) RELOC_SCAN_VGPR_ATTR void k_db_scan(
    const uint4 *__restrict__ db, const int64_t *__restrict__ off, const int32_t *__restrict__ rec_ids,
    const int32_t *__restrict__ n_ids_p, int n_ids_max, const uint4 *__restrict__ cur,
    const int32_t *__restrict__ n_cur_p, int n_cur_max, int max_rows, int32_t *__restrict__ counts, ScanMask mask, u32 *ticket,
    int quota, int n_bounded, int col_words)
{
    extern __shared__ u32 lds[];
    const int C = n_cur_p ? min(*n_cur_p, n_cur_max) : n_cur_max;
    db_count_body<NJ>(lds, C, db, off, rec_ids, n_ids_p, n_ids_max, cur, max_rows, counts, mask, ticket, quota, n_bounded, col_words);
}

// One frame's emit pass, NW waves per workgroup (see launch_db_emit).  Plain pointer arguments: a frame struct costs registers here.
template <int NJ, int NW>
__global__ __launch_bounds__(64 * NW, 16 / NW) RELOC_SCAN_VGPR_ATTR void k_db_scan_emit(
    const uint4 *__restrict__ db, const int64_t *__restrict__ off, const int32_t *__restrict__ rec_ids,
    const int32_t *__restrict__ n_ids_p, int n_ids_max, const uint4 *__restrict__ cur,
    const int32_t *__restrict__ n_cur_p, int n_cur_max, int max_rows, int32_t *__restrict__ m_qidx,
    int32_t *__restrict__ m_tidx, int32_t *__restrict__ m_dist, int32_t *__restrict__ m_n, int emit_stride,
    const float *__restrict__ g_pts3d, const float *__restrict__ g_xy, float *__restrict__ g_obj, float *__restrict__ g_img)
{
    extern __shared__ u32 lds[];
    RELOC_SMALL_KERNEL_PRIO();          // the emit pass of a few candidates is one of the tick's small kernels
    const int C = n_cur_p ? min(*n_cur_p, n_cur_max) : n_cur_max;
    db_emit_body<NJ, NW>(lds, C, db, off, rec_ids, n_ids_p, n_ids_max, cur, max_rows, m_qidx, m_tidx, m_dist, m_n, emit_stride, g_pts3d,
                         g_xy, g_obj, g_img);
}

// The emit pass (match lists of the candidate records, M:327-336) of up to 8 frames in one launch: blockIdx.y = frame.
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

__global__ __launch_bounds__(256, 4) RELOC_SCAN_VGPR_ATTR void k_db_scan_emit_batch(const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_ids_max,
                                                          int n_cur_max, int max_rows, int emit_stride, const float *__restrict__ g_pts3d,
                                                          EmitBatch bt)
{
    extern __shared__ u32 lds[];
    RELOC_SMALL_KERNEL_PRIO();
    const EmitFrame &F = bt.f[blockIdx.y];
    const int C = F.n_cur_p ? min(*F.n_cur_p, n_cur_max) : n_cur_max;
    db_emit_body<8, 4>(lds, C, db, off, F.rec_ids, F.n_ids_p, n_ids_max, F.cur, max_rows, F.m_qidx, F.m_tidx, F.m_dist, F.m_n, emit_stride,
                       g_pts3d, F.g_xy, F.g_obj, F.g_img);
}

// Dynamic LDS of a scan workgroup: col_words words of column minima, a row key per teach row, 16 words of counters and, for
// the counting scan, slice_keys 16-bit keys of per-wave column minima behind them (db_count_body)
static int scan_lds_bytes(const char *who, int col_words, int max_rows, size_t &lds, int slice_keys = 0)
{
    lds = (size_t)(col_words + max_rows + 16) * 4 + (size_t)slice_keys * 2;
    if (lds > 160 * 1024) { reloc_set_error("%s: LDS demand %zu bytes", who, lds); return RELOC_E_CAPACITY; }
    return RELOC_OK;
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

__global__ __launch_bounds__(256, 4) RELOC_SCAN_VGPR_ATTR void k_db_scan_batch(const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_ids,
                                                          int n_cur_max, int max_rows, ScanBatch bt, u32 *ticket_pool, int quota, int n_bounded, int col_words)
{
    extern __shared__ u32 lds[];
    const int f = blockIdx.x % bt.n;                       // workgroup-uniform
    ScanMask mask;
    mask.xyh = bt.xyh;
    for (int k = 0; k < 4; ++k) mask.q[k] = bt.q[f][k];
    mask.cos_tol = bt.cos_tol;
    mask.skip_if = bt.skip_if[f];
    const int C = bt.n_cur[f] ? min(*bt.n_cur[f], n_cur_max) : n_cur_max;
    db_count_body<8>(lds, C, db, off, nullptr, nullptr, n_ids, bt.cur[f], max_rows, bt.counts[f], mask, ticket_pool + f * 8 * TICKET_STRIDE, quota,
                     n_bounded, col_words, ticket_pool, bt.n, (int)(blockIdx.x / bt.n), (int)((gridDim.x + bt.n - 1 - f) / bt.n));
}

// ---------------------------------------------------------------------------------------------
// Ratio-test score of every record (reference _archive/anchor_localizer.py:82-90,
// checkpoint_a_selftest.py:68-71): per record, the number of current descriptors whose two nearest rows
// of the record satisfy d1 < ratio * d2.  Same data flow as k_db_scan (512 current descriptors per wave
// in registers, teach rows through the scalar cache) but the epilogue only tracks the two smallest
// distances per column: v_max_u16 + 2 v_min_u16 per pair, no indices, no cross-lane work in the loop.
__device__ __forceinline__ u32 max_u16(u32 a, u32 b)
{
    u32 r;
    asm("v_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

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
    const int C = n_cur_p ? min(*n_cur_p, n_cur_max) : n_cur_max;
    db_ratio_body<TICK>(db, off, n_rec, cur, C, ratio, counts, mask, min_rows, blockIdx.x, gridDim.x);
}

// the ratio scans of up to 8 frames in one launch: blockIdx.y = frame, which counts into bt.counts[frame] (ScanBatch)
__global__ __launch_bounds__(256, 4) void k_db_ratio_batch(const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_rec,
                                                           int n_cur_max, double ratio, ScanBatch bt, int min_rows)
{
    const int f = blockIdx.y;
    ScanMask mask;
    mask.xyh = bt.xyh;
    for (int k = 0; k < 4; ++k) mask.q[k] = bt.q[f][k];
    mask.cos_tol = bt.cos_tol;
    mask.skip_if = bt.skip_if[f];
    const int C = bt.n_cur[f] ? min(*bt.n_cur[f], n_cur_max) : n_cur_max;
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
    const int C = F.n_cur_p ? min(*F.n_cur_p, n_cur_max) : n_cur_max;
    db_ratio_emit_body<NW>(C, db, off, n_ids_max, ratio, min_rows, gate_off, emit_stride, g_pts3d, F);
}

// the same for up to 8 frames in one launch: blockIdx.y = frame
__global__ __launch_bounds__(256) void k_db_ratio_emit_batch(const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_ids_max,
                                                             int n_cur_max, double ratio, int min_rows, int gate_off, int emit_stride,
                                                             const float *__restrict__ g_pts3d, EmitBatch bt)
{
    RELOC_SMALL_KERNEL_PRIO();
    const EmitFrame &F = bt.f[blockIdx.y];
    const int C = F.n_cur_p ? min(*F.n_cur_p, n_cur_max) : n_cur_max;
    db_ratio_emit_body<4>(C, db, off, n_ids_max, ratio, min_rows, gate_off, emit_stride, g_pts3d, F);
}

// ---------------------------------------------------------------------------------------------
// Few current descriptors (C <= 64): the roles swap.  With one or a few dozen queries the column-per-lane kernel
// above wastes its 128 lanes x columns (Q = 1 and Q = 32 both cost the 128-column price, 55 us at 10 000 x 64); here a
// LANE is a teach row -- the wave reads 64 rows of the record straight from HBM (2 KB, coalesced), the queries are
// wave-uniform and arrive through the scalar cache -- so the work follows C and the kernel runs at the pace of the
// database read up to Q ~ 8.  One wave owns a record (no barriers); the SIMD's eight waves hide each other's HBM latency
// (one record per wave turn: taking two or four per turn lets the SIMD's waves fall into step, profiles/r3_small_q_records_per_turn.log).
// Records of more than SQ_MAX_ROWS rows, emit mode and the heading mask stay with k_db_scan.
constexpr int SQ_MAX_ROWS = 1024;
constexpr int SQ_WAVES = 4;

// ---- few-query scan, round 4 -------------------------------------------------------------------------------------------
// Round 4 rebuilt the kernel for fewer instructions per record (round 3's form: profiles/r3_*, git history):
//   (1) the distances of four queries run as EIGHT accumulator chains (query x descriptor half) in the pinned xor -> bcnt
//       order of ham8_cols (see there: a v_bcnt must not meet an accumulator written fewer than ~16 instructions earlier);
//       the two halves are merged and shifted by one v_add_lshl_u32;
//   (2) the butterfly that takes each query's best row over the 64 lanes is built from v_min_u16 WITH the DPP lane exchange
//       in the instruction (round 3: v_mov_dpp + two v_cndmask + v_min per node): a node that splits on lane bit 2 or 3 is two
//       bank-masked DPP minima, on bit 4 or 5 a v_permlane swap and a minimum, and the bits that are left are reduced on ONE
//       value -- 19 instead of ~36 instructions for 8 queries, 32 instead of ~70 for 16 (sq_bfly);
//   (3) the best row of every query lives in ONE register (lane sq_lane_of(q) holds query q: the butterfly leaves the
//       group's minima on every lane whose bits 2.. spell the query, so that lane takes its own), and a row's mutual test
//       fetches its query's entry with one ds_bpermute: no LDS arrays for records of up to 64 rows, one 16-bit LDS word
//       per row beyond that.
// (Requesting the next record's rows one record ahead: measured and dropped, profiles/README.md "Dropped experiments" #5.)
__device__ __forceinline__ u32 add_lshl6(u32 a, u32 b)
{
    u32 r;
    asm("v_add_lshl_u32 %0, %1, %2, 6" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// hs[j] = distance(query j, row) << 6 for four queries whose words are wave-uniform (SGPRs)
__device__ __forceinline__ void sq_dist4(const u32 (&qw)[4][8], const u32 (&w)[8], u32 (&hs)[4])
{
    u32 acc[4][2];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                u32 x;
                asm volatile("v_xor_b32 %0, %1, %2" : "=v"(x) : "s"(qw[j][4 * h + k]), "v"(w[4 * h + k]));
                if (k == 0) asm volatile("v_bcnt_u32_b32 %0, %1, 0" : "=v"(acc[j][h]) : "v"(x));
                else asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc[j][h]) : "v"(x));
            }
#pragma unroll
    for (int j = 0; j < 4; ++j) hs[j] = add_lshl6(acc[j][0], acc[j][1]);
}

// four queries' words (32 SGPRs) by scalar loads at 32-bit byte offsets from the wave-uniform base; indices past the last
// query repeat it (a duplicate offers the same distance with a larger index: it never wins a minimum)
__device__ __forceinline__ void sq_load4(const uint4 *__restrict__ cur, int q0, int C, u32 (&qw)[4][8])
{
    const char *base = (const char *)cur;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const u32 o = (u32)min(q0 + jj, C - 1) << 5;
        const uint4 qa = *(const uint4 *)(base + o), qb = *(const uint4 *)(base + o + 16);
        qw[jj][0] = qa.x; qw[jj][1] = qa.y; qw[jj][2] = qa.z; qw[jj][3] = qa.w;
        qw[jj][4] = qb.x; qw[jj][5] = qb.y; qw[jj][6] = qb.z; qw[jj][7] = qb.w;
    }
}

// Butterfly minimum of G 16-bit keys per lane over the 64 lanes: afterwards EVERY lane l holds the minimum over all lanes of
// vector j(l) = (l >> 2) & (G - 1).  One asm statement: the order is fixed, so the wait states the hardware does not
// interlock are counted by hand (a VALU write of a register -> a DPP or v_permlane read of it needs 2 wait states: the
// producer is never closer than two instructions, or an s_nop 1 stands between; the opening s_nop covers the compiler's
// instruction in front of the statement).  Nodes:  lane bit 2: bank-masked row_shl:4 / row_shr:4;  bit 3: row_ror:8;
// bit 4 / 5: v_permlane16/32_swap (a half exchange: one operand's odd halves against the other's even halves) + minimum;
// bits left over are reduced on the one remaining value (quad_perm for bits 0 and 1; a swap with a copy for bits 4, 5).
#define SQ_N4(a, b)  "v_min_u16_dpp " a ", " a ", " a " row_shl:4 row_mask:0xf bank_mask:0x5\n\t" \
                     "v_min_u16_dpp " a ", " b ", " b " row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
#define SQ_N8(a, b)  "v_min_u16_dpp " a ", " a ", " a " row_ror:8 row_mask:0xf bank_mask:0x3\n\t" \
                     "v_min_u16_dpp " a ", " b ", " b " row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
#define SQ_Q1(a)     "v_min_u16_dpp " a ", " a ", " a " quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
#define SQ_Q2(a)     "v_min_u16_dpp " a ", " a ", " a " quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
#define SQ_NOP       "s_nop 1\n\t"
template <int G>
__device__ __forceinline__ u32 sq_bfly(u32 (&d)[G])
{
    if constexpr (G == 16) {
        asm volatile(SQ_NOP
                     SQ_N4("%0", "%1") SQ_N4("%2", "%3") SQ_N4("%4", "%5") SQ_N4("%6", "%7")
                     SQ_N4("%8", "%9") SQ_N4("%10", "%11") SQ_N4("%12", "%13") SQ_N4("%14", "%15")
                     SQ_N8("%0", "%2") SQ_N8("%4", "%6") SQ_N8("%8", "%10") SQ_N8("%12", "%14")
                     "v_permlane16_swap_b32 %0, %4\n\t"              // %4 was written 5 instructions ago
                     "v_permlane16_swap_b32 %8, %12\n\t"             // %12: the instruction before last + one swap: pad
                     "v_min_u16 %0, %0, %4\n\t"
                     "v_min_u16 %8, %8, %12\n\t"
                     SQ_NOP
                     "v_permlane32_swap_b32 %0, %8\n\t"
                     "v_min_u16 %0, %0, %8\n\t"
                     SQ_NOP SQ_Q1("%0") SQ_NOP SQ_Q2("%0")
                     : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4]), "+v"(d[5]), "+v"(d[6]), "+v"(d[7]), "+v"(d[8]),
                       "+v"(d[9]), "+v"(d[10]), "+v"(d[11]), "+v"(d[12]), "+v"(d[13]), "+v"(d[14]), "+v"(d[15]));
    } else if constexpr (G == 8) {
        asm volatile(SQ_NOP
                     SQ_N4("%0", "%1") SQ_N4("%2", "%3") SQ_N4("%4", "%5") SQ_N4("%6", "%7")
                     SQ_N8("%0", "%2") SQ_N8("%4", "%6")
                     SQ_NOP
                     "v_permlane16_swap_b32 %0, %4\n\t"
                     "v_min_u16 %0, %0, %4\n\t"
                     SQ_NOP SQ_Q1("%0") SQ_NOP SQ_Q2("%0")
                     "v_mov_b32 %4, %0\n\t"
                     SQ_NOP
                     "v_permlane32_swap_b32 %0, %4\n\t"
                     "v_min_u16 %0, %0, %4\n\t"
                     : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4]), "+v"(d[5]), "+v"(d[6]), "+v"(d[7]));
    } else {
        static_assert(G == 4, "groups of 4, 8 or 16 queries");
        asm volatile(SQ_NOP
                     SQ_N4("%0", "%1") SQ_N4("%2", "%3")
                     SQ_NOP
                     SQ_N8("%0", "%2")
                     SQ_NOP SQ_Q1("%0") SQ_NOP SQ_Q2("%0")
                     "v_mov_b32 %2, %0\n\t"
                     SQ_NOP
                     "v_permlane16_swap_b32 %0, %2\n\t"
                     "v_min_u16 %0, %0, %2\n\t"
                     "v_mov_b32 %2, %0\n\t"
                     SQ_NOP
                     "v_permlane32_swap_b32 %0, %2\n\t"
                     "v_min_u16 %0, %0, %2\n\t"
                     : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]));
    }
    return d[0];
}
#undef SQ_N4
#undef SQ_N8
#undef SQ_Q1
#undef SQ_Q2
#undef SQ_NOP
// the lane whose register holds query q's entry: bits 2.. = q's place in its group (what sq_bfly leaves there), the group
// number in the lane bits the butterfly reduced over
template <int G>
__device__ __forceinline__ u32 sq_lane_of(u32 q)
{
    if constexpr (G == 16) return ((q & 15u) << 2) | (q >> 4);                          // 4 groups: bits 0, 1
    else if constexpr (G == 8) return ((q & 7u) << 2) | ((q >> 3) & 3u) | (q & 32u);     // 8 groups: bits 0, 1, 5
    else return (q & 3u) << 2;
}

template <int G, bool HOIST>
__global__ __launch_bounds__(64 * SQ_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_db_scan_rows(
    const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_rec, const uint4 *__restrict__ cur,
    const int32_t *__restrict__ n_cur_p, int n_cur_max, int32_t *__restrict__ counts)
{
    __shared__ unsigned short s_row[SQ_WAVES][SQ_MAX_ROWS];   // per row: distance << 6 | query of the best query (records > 64 rows)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int C = n_cur_p ? min(*n_cur_p, n_cur_max) : n_cur_max;
    unsigned short *rowk = s_row[wave];
    const int gw = blockIdx.x * SQ_WAVES + wave, nw = gridDim.x * SQ_WAVES;
    // the group whose entries this lane keeps (see sq_lane_of): the lane bits the butterfly reduces over
    const int my_group = G == 16 ? (lane & 3) : (G == 8 ? ((lane & 3) | ((lane >> 5) << 2)) : 0);
    constexpr int NH = HOIST ? G : 1;
    u32 qs[NH][8];
    if constexpr (HOIST) {
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int q = max(min(j, C - 1), 0);        // wave-uniform; repeats of the last query lose every tie (larger index)
            const uint4 qa = cur[2 * q], qb = cur[2 * q + 1];                // scalar loads, once
            qs[j][0] = qa.x; qs[j][1] = qa.y; qs[j][2] = qa.z; qs[j][3] = qa.w;
            qs[j][4] = qb.x; qs[j][5] = qb.y; qs[j][6] = qb.z; qs[j][7] = qb.w;
        }
    }
    // one 64-row chunk (rows tc .. tc + 63 in the lanes) against all queries: updates colk, returns the rows' best queries
    auto chunk = [&](const uint4 a, const uint4 b, int tc, u32 &colk) -> u32 {
        const u32 w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        u32 rbest = 0xFFFFu;
        for (int q0 = 0; q0 < (HOIST ? 1 : C); q0 += G) {
            u32 ck[G];
#pragma unroll
            for (int j4 = 0; j4 < G; j4 += 4) {
                u32 hs[4];
                if constexpr (HOIST) {
                    const u32 (&qv)[4][8] = *reinterpret_cast<const u32 (*)[4][8]>(&qs[j4 < NH ? j4 : 0]);
                    sq_dist4(qv, w, hs);
                } else {
                    u32 qw[4][8];
                    sq_load4(cur, q0 + j4, C, qw);
                    sq_dist4(qw, w, hs);
                }
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    rbest = min_u16(rbest, hs[jj] | (u32)(q0 + j4 + jj));     // distance <= 256: (256 << 6 | 63) < 2^15
                    ck[j4 + jj] = hs[jj] | (u32)lane;
                }
            }
            const u32 m = sq_bfly<G>(ck);               // EVERY lane l: best (distance, lane) of query q0 + ((l >> 2) & (G - 1)) over the 64 rows
            const u32 key = ((m >> 6) << 16) | (u32)(tc + (int)(m & 63u));
            const u32 better = umin(colk, key);
            colk = my_group * G == q0 ? better : colk;                     // the lane of this group keeps the entry of its query
        }
        return rbest;
    };
    for (int r = gw; r < n_rec; r += nw) {
        const int64_t row0 = off[r];
        const int n = (int)(off[r + 1] - row0);
        if (n <= 0 || C <= 0) {
            if (lane == 0) counts[r] = 0;
            continue;
        }
        const uint4 *rec = db + 2 * row0;
        u32 colk = 0xFFFFFFFFu;                          // lane sq_lane_of(q): distance << 16 | row of query q's best row so far
        // mutual pairs: row t's best query must name t as its best row (lowest index on ties both ways)
        int total;
        {
            const int row = min(lane, n - 1);            // lanes past the end repeat the last row (larger lane index: loses every tie)
            const u32 rb = chunk(rec[2 * row], rec[2 * row + 1], 0, colk);
            if (n <= 64) {
                const u32 peer = (u32)__builtin_amdgcn_ds_bpermute((int)(sq_lane_of<G>(rb & 63u) << 2), (int)colk);
                total = __popcll(__ballot(lane < n && (peer & 0xFFFFu) == (u32)lane));
                if (lane == 0) counts[r] = total;
                continue;
            }
            rowk[lane] = (unsigned short)rb;
        }
        for (int tc = 64; tc < n; tc += 64) {                              // records of more than 64 rows: further chunks
            const int row = min(tc + lane, n - 1);
            const u32 rb = chunk(rec[2 * row], rec[2 * row + 1], tc, colk);
            if (tc + lane < n) rowk[tc + lane] = (unsigned short)rb;
        }
        total = 0;
        for (int tc = 0; tc < n; tc += 64) {
            const u32 k = tc + lane < n ? rowk[tc + lane] : 0u;
            const u32 peer = (u32)__builtin_amdgcn_ds_bpermute((int)(sq_lane_of<G>(k & 63u) << 2), (int)colk);
            total += __popcll(__ballot(tc + lane < n && (peer & 0xFFFFu) == (u32)(tc + lane)));
        }
        if (lane == 0) counts[r] = total;
    }
}

// Launch plan of a counting scan of the context's database (k_db_scan<NJ>, k_db_scan_batch): 4-wave workgroups
// over column blocks of 64 * nj current descriptors, n_cur_max of them at most.
struct CountPlan {
    int col_words = 0;            // column minima: one buffer for the capacity; the kernel double-buffers inside it when the
                                  // run-time count leaves room (db_count_body), so at least two column blocks
    size_t lds = 0;
    int resident = 0;             // workgroups resident on the chip: 4 per CU (16 waves, 128-VGPR kernel) unless their LDS does not fit
    int quota = 0, n_bounded = 0; // row budget of the first n_bounded workgroups of a scan (0, 0: none, see db_count_body)

    int init(const reloc_ctx *ctx, const char *who, int nj, int n_cur_max, int max_rows)
    {
        const int cb = 64 * nj, ncb = (n_cur_max + cb - 1) / cb;
        col_words = (ncb >= 2 ? ncb : 2) * cb;
        // + the four waves' slices of one column block, 4 KB at nj = 8: with the 32 KB of a context made for 8192 features
        // four workgroups still fit a CU's 160 KB up to records of 1008 rows
        if (int rc = scan_lds_bytes(who, col_words, max_rows, lds, 4 * cb)) return rc;
        const int wg_per_cu = (int)(160 * 1024 / lds);
        resident = ctx->num_cu * (wg_per_cu < 4 ? wg_per_cu : 4);
        return RELOC_OK;
    }

    // `workgroups` workgroups per scan with a budget of ROWS each, together the whole database (q_rec records' worth at the
    // average record size); the caller adds the sweepers behind them, which draw until the counters are dry
    void budget(const reloc_ctx *ctx, int workgroups)
    {
        const DbArena &db = ctx_db(ctx);
        const int n_ids = (int)db.records;
        if (workgroups > n_ids) workgroups = n_ids;
        if (workgroups < 1) workgroups = 1;
        const int q_rec = (n_ids + workgroups - 1) / workgroups;
        n_bounded = (n_ids + q_rec - 1) / q_rec;
        quota = (int)((db.rows * q_rec + n_ids - 1) / n_ids);
        if (quota < 1) quota = 1;
    }
};

// The counters of a context's whole-database scans (ctx->scan_ticket), zero whenever no scan is running: the last workgroup to
// leave zeroes them again.
int scan_alloc(reloc_ctx *ctx)
{
    if (int rc = ctx_dev_alloc(ctx, &ctx->scan_ticket, SCAN_TICKET_WORDS)) return rc;
    HIP_TRY(hipMemset(ctx->scan_ticket, 0, SCAN_TICKET_WORDS * sizeof(uint32_t)));
    return RELOC_OK;
}

// The whole-database scan of one frame.  Records are DRAWN from per-XCD ticket counters instead of dealt round-robin, so the
// work stays balanced to the last record, by ONE resident generation of workgroups that draws until the counters are dry:
// the fastest form alone (152 us where one generation with row budgets takes 177: static shares leave a tail) and, since the
// scan leaves 96 registers per lane to the kernels of other streams, beside them as well (4 streams: 6 826 frames/s against
// 6 853 / 6 759 / 6 752 / 6 604 with 1 / 2 / 3 / 4 generations of budgets, profiles/r4_scan_generations.log; the other forms
// dropped on the way: profiles/README.md "Dropped experiments" #4, #6).  RELOC_SCAN_GENS=n > 0 (developer switch) runs the
// form of a batched launch instead: n generations of workgroups with row budgets and one sweeper per XCD.  The 128- and
// 256-column kernels (their short records do not cover the draw latency) and databases that do not fill the chip are dealt
// statically.
int launch_db_count(reloc_ctx *ctx, const uint8_t *cur, const int32_t *n_cur_dev, int n_cur_max, int32_t *counts, const ScanMask &mask)
{
    const DbArena &db = ctx_db(ctx);
    const int n_ids = (int)db.records;
    if (n_ids <= 0) return RELOC_OK;
    if (n_cur_max > 65535) { reloc_set_error("db scan: more than 65535 current descriptors"); return RELOC_E_CAPACITY; }
    if (db.max_rows > MAX_REC_ROWS) { reloc_set_error("db scan: record larger than %d rows", MAX_REC_ROWS); return RELOC_E_CAPACITY; }
    const int max_rows = db.max_rows < 1 ? 1 : db.max_rows;
    const uint4 *desc = (const uint4 *)db.desc;
    if (!mask.xyh && n_cur_max <= 64 && max_rows <= SQ_MAX_ROWS) {
        // few queries: lane = teach row (k_db_scan_rows)
        if (n_cur_max == 0) {                              // a capacity of zero descriptors: nothing may be read from `cur`
            HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_ids * sizeof(int32_t), ctx->stream));
            return RELOC_OK;
        }
        int grid = ctx->num_cu * 8;                        // 8 workgroups of 4 waves per CU
        const int need = (n_ids + SQ_WAVES - 1) / SQ_WAVES;
        if (grid > need) grid = need;
#define RELOC_LAUNCH_ROWS(G, HOIST)                                                                                           \
    hipLaunchKernelGGL((k_db_scan_rows<G, HOIST>), dim3(grid), dim3(64 * SQ_WAVES), 0, ctx->stream, desc, db.off, n_ids, \
                       (const uint4 *)cur, n_cur_dev, n_cur_max, counts)
        // G = queries per butterfly group: a call with 1-4 queries evaluates 4 distances per row, not 16; its query words stay in SGPRs
        if (n_cur_max <= 4) RELOC_LAUNCH_ROWS(4, true); else if (n_cur_max <= 8) RELOC_LAUNCH_ROWS(8, false); else RELOC_LAUNCH_ROWS(16, false);
#undef RELOC_LAUNCH_ROWS
        HIP_TRY(hipGetLastError());
        return RELOC_OK;
    }
    const int nj = n_cur_max <= 128 ? 2 : (n_cur_max <= 256 ? 4 : 8);      // columns per lane, see k_db_scan
    CountPlan p;
    if (int rc = p.init(ctx, "db scan", nj, n_cur_max, max_rows)) return rc;
    int grid = ctx->num_cu * 16;
    u32 *ticket = nullptr;
    if (nj == 8 && n_ids > p.resident && ctx->scan_ticket) {
        ticket = ctx->scan_ticket;
        grid = p.resident;
        if (ctx->scan_gens > 0) {
            p.budget(ctx, p.resident * ctx->scan_gens);
            grid = p.n_bounded + 8;                                               // + one sweeper per XCD
        }
    }
    if (grid > n_ids) grid = n_ids;
#define RELOC_LAUNCH_COUNT(NJ)                                                                                               \
    hipLaunchKernelGGL((k_db_scan<NJ>), dim3(grid), dim3(256), p.lds, ctx->stream, desc, db.off, nullptr, nullptr, n_ids,       \
                       (const uint4 *)cur, n_cur_dev, n_cur_max, max_rows, counts, mask, ticket, p.quota, p.n_bounded, p.col_words)
    if (nj == 2) RELOC_LAUNCH_COUNT(2); else if (nj == 4) RELOC_LAUNCH_COUNT(4); else RELOC_LAUNCH_COUNT(8);
#undef RELOC_LAUNCH_COUNT
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

// Match lists of a few records, dealt statically.  One workgroup per record is alone on its CU and one wave per SIMD issues an
// instruction only every ~7 cycles, so the record's rows are the kernel's run time.  8 waves per record take the synchronous
// tick from 322 / 152 to 318 / 149 us (global / local) -- and the 4-stream whole-database run from 5940 to 5360 frames/s: a
// 512-thread workgroup of this register size needs TWO scan workgroups of one CU to retire before it fits.  So: 8 waves where
// no scan runs beside it (latency: local-candidate ticks, single calls), 4 waves in ticks that scan the database.
// Frame f lists the records rec_ids (n_ids_max capacity, count on the device at n_ids_p when non-NULL; rec_ids == NULL:
// records 0..n_ids_max-1) of the database db_desc / db_off against its current descriptors (n_cur_max capacity), emit_stride
// apart; with g_obj set every match also leaves its 3-D / 2-D pair (db_emit_body).  A batch runs the 8-column kernel.
static int launch_db_emit(reloc_ctx *const *ctxs, int n, const EmitBatch &bt, const uint8_t *db_desc, const int64_t *db_off,
                          int max_rows, const float *g_pts3d, int n_ids_max, int n_cur_max, int emit_stride, bool latency)
{
    reloc_ctx *c0 = ctxs[0];
    if (n < 1 || n > RELOC_BATCH_MAX) { reloc_set_error("emit: 1..%d frames", RELOC_BATCH_MAX); return RELOC_E_ARG; }
    if (n_ids_max <= 0) return RELOC_OK;
    if (n_cur_max > 65535) { reloc_set_error("db scan: more than 65535 current descriptors"); return RELOC_E_CAPACITY; }
    if (max_rows > MAX_REC_ROWS) { reloc_set_error("db scan: record larger than %d rows", MAX_REC_ROWS); return RELOC_E_CAPACITY; }
    if (max_rows < 1) max_rows = 1;
    const int nj = n > 1 || n_cur_max > 256 ? 8 : (n_cur_max <= 128 ? 2 : 4);      // columns per lane, see k_db_scan
    const int cb = 64 * nj;
    const int ncb = (n_cur_max + cb - 1) / cb > 0 ? (n_cur_max + cb - 1) / cb : 1;
    size_t lds;
    if (int rc = scan_lds_bytes("db scan", ncb * cb, max_rows, lds)) return rc;
    const int grid = n_ids_max < c0->num_cu * 16 ? n_ids_max : c0->num_cu * 16;
    if (n == 1) {
        const EmitFrame &F = bt.f[0];
#define RELOC_LAUNCH_EMIT(NJ, NW)                                                                                            \
    hipLaunchKernelGGL((k_db_scan_emit<NJ, NW>), dim3(grid), dim3(64 * NW), lds, c0->stream, (const uint4 *)db_desc, db_off, F.rec_ids, \
                       F.n_ids_p, n_ids_max, F.cur, F.n_cur_p, n_cur_max, max_rows, F.m_qidx, F.m_tidx, F.m_dist, F.m_n, emit_stride, \
                       g_pts3d, F.g_xy, F.g_obj, F.g_img)
        if (latency) {
            if (nj == 2) RELOC_LAUNCH_EMIT(2, 8); else if (nj == 4) RELOC_LAUNCH_EMIT(4, 8); else RELOC_LAUNCH_EMIT(8, 8);
        } else {
            if (nj == 2) RELOC_LAUNCH_EMIT(2, 4); else if (nj == 4) RELOC_LAUNCH_EMIT(4, 4); else RELOC_LAUNCH_EMIT(8, 4);
        }
#undef RELOC_LAUNCH_EMIT
    } else {
        hipLaunchKernelGGL(k_db_scan_emit_batch, dim3(grid, n), dim3(256), lds, c0->stream, (const uint4 *)db_desc, db_off, n_ids_max,
                           n_cur_max, max_rows, emit_stride, g_pts3d, bt);
    }
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

// The emit pass under RELOC_MATCH_RATIO: launch_db_emit's arguments and shapes (8 waves for latency, 4 beside scans, the batch
// kernel for several frames) with the ratio and the record-length gate of the tick (min_rows, gate_off: db_ratio_emit_body).
// A list holds up to n_cur_max entries, so that many must fit the list stride.
static int launch_db_ratio_emit(reloc_ctx *const *ctxs, int n, const EmitBatch &bt, const uint8_t *db_desc, const int64_t *db_off,
                                const float *g_pts3d, int n_ids_max, int n_cur_max, int emit_stride, double ratio, int min_rows,
                                int gate_off, bool latency)
{
    reloc_ctx *c0 = ctxs[0];
    if (n < 1 || n > RELOC_BATCH_MAX) { reloc_set_error("emit: 1..%d frames", RELOC_BATCH_MAX); return RELOC_E_ARG; }
    if (n_ids_max <= 0) return RELOC_OK;
    if (n_cur_max > 65535) { reloc_set_error("db scan: more than 65535 current descriptors"); return RELOC_E_CAPACITY; }
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

int launch_tick_emit(reloc_ctx *const *ctxs, int n, bool latency)
{
    reloc_ctx *c0 = ctxs[0];
    const DbArena &db = ctx_db(c0);
    EmitBatch bt;
    frame_slots(ctxs, n, [&](int f, reloc_ctx *c, int) { bt.f[f] = emit_frame(c); });
    if (c0->match.ratio_on())
        return launch_db_ratio_emit(ctxs, n, bt, db.desc, db.off, db.pts3d, MAX_CAND, c0->max_feat, MAX_REC_ROWS, c0->match.ratio,
                                    c0->prm.min_matches, MAX_CAND, latency);
    return launch_db_emit(ctxs, n, bt, db.desc, db.off, db.max_rows, db.pts3d, MAX_CAND, c0->max_feat, MAX_REC_ROWS, latency);
}

// One launch for the whole-database scans of n contexts that share a stream and a database (ctxs[0]'s is scanned):
// frame f = ctxs[f]'s current features, counts into the counts of ctxs[f]'s arena.  q: n x 4 base_link quaternions (heading mask),
// auto_mode: frames whose local search found candidates stand down on the device.
int launch_db_scan_batch(reloc_ctx *const *ctxs, int n, const double *q, double cos_tol, bool auto_mode, bool heading_mask)
{
    reloc_ctx *c0 = ctxs[0];
    if (n < 1 || n > RELOC_BATCH_MAX) { reloc_set_error("scan batch: 1..%d frames", RELOC_BATCH_MAX); return RELOC_E_ARG; }
    const DbArena &db = ctx_db(c0);
    if (c0->max_feat > 65535 || db.max_rows > MAX_REC_ROWS) { reloc_set_error("scan batch: capacity"); return RELOC_E_CAPACITY; }
    const int n_ids = (int)db.records, max_rows = db.max_rows < 1 ? 1 : db.max_rows;
    // n_cur_max = the feature capacity; the 8-column kernel walks column blocks of 512 (one block for nfeatures <= 512)
    CountPlan p;
    if (int rc = p.init(c0, "scan batch", 8, c0->max_feat, max_rows)) return rc;
    ScanBatch bt;
    bt.n = n;
    bt.xyh = heading_mask ? db.xy_heading : nullptr;
    bt.cos_tol = cos_tol;
    frame_slots(ctxs, n, [&](int f, reloc_ctx *c, int g) {
        bt.cur[f] = (const uint4 *)c->orb.buf.f_desc; bt.n_cur[f] = c->orb.buf.f_count; bt.counts[f] = ctx_db(c).counts;
        bt.skip_if[f] = auto_mode ? c->tick.cand_n : nullptr;
        for (int k = 0; k < 4; ++k) bt.q[f][k] = q[4 * g + k];
    });
    // `gens` generations in all (not per frame): a workgroup's budget grows with the batch, and with it the share of the
    // launch that is not prologue.  Per frame: the budgeted workgroups + one sweeper behind them
    const int gens = c0->scan_gens > 0 ? c0->scan_gens : 1;
    p.budget(c0, (p.resident * gens + n - 1) / n);
    const int per_frame = p.n_bounded + 1 < n_ids ? p.n_bounded + 1 : n_ids;
    hipLaunchKernelGGL(k_db_scan_batch, dim3(per_frame * n), dim3(256), p.lds, c0->stream, (const uint4 *)db.desc, db.off,
                       n_ids, c0->max_feat, max_rows, bt, c0->scan_ticket, p.quota, p.n_bounded, p.col_words);
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
    if (c0->max_feat > 65535) { reloc_set_error("ratio scan: more than 65535 current descriptors"); return RELOC_E_CAPACITY; }
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
        ScanBatch bt;
        bt.n = n;
        bt.xyh = base_poses ? db.xy_heading : nullptr;
        bt.cos_tol = cos_tol;
        frame_slots(ctxs, n, [&](int f, reloc_ctx *c, int g) {
            bt.cur[f] = (const uint4 *)c->orb.buf.f_desc; bt.n_cur[f] = c->orb.buf.f_count; bt.counts[f] = ctx_db(c).counts;
            bt.skip_if[f] = auto_mode ? c->tick.cand_n : nullptr;
            for (int k = 0; k < 4; ++k) bt.q[f][k] = base_poses ? base_poses[7 * g + 3 + k] : (k == 3 ? 1.0 : 0.0);
        });
        hipLaunchKernelGGL(k_db_ratio_batch, dim3(grid, n), dim3(256), 0, c0->stream, desc, db.off, n_ids, c0->max_feat, c0->match.ratio,
                           bt, c0->prm.min_matches);
    }
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

// ---------------------------------------------------------------------------------------------
// Generic two-nearest-neighbour search: lane = one row of A, B rows stream through the scalar
// cache.  key = distance << 22 | index (nb < 2^22).  grid.x tiles A rows, grid.y splits B.
// Partial results (2 keys per A row per split) are merged by k_knn2_merge.
__global__ __launch_bounds__(256) void k_knn2(const uint4 *__restrict__ A, int na, const uint4 *__restrict__ B,
                                              int nb, int rows_per_split, u32 *__restrict__ part)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j0 = blockIdx.y * rows_per_split;
    const int j1 = min(nb, j0 + rows_per_split);
    u32 q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < na) {
        const uint4 a = A[2 * i], b = A[2 * i + 1];
        q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w;
        q[4] = b.x; q[5] = b.y; q[6] = b.z; q[7] = b.w;
    }
    u32 k0 = 0xFFFFFFFFu, k1 = 0xFFFFFFFFu;
#pragma unroll 4
    for (int j = j0; j < j1; ++j) {
        const u32 h = ham8(q, B[2 * j], B[2 * j + 1], 0);
        const u32 key = (h << 22) | (u32)j;
        const u32 m = umax(k0, key);
        k0 = umin(k0, key);
        k1 = umin(k1, m);
    }
    if (i < na) {
        part[((size_t)blockIdx.y * na + i) * 2] = k0;
        part[((size_t)blockIdx.y * na + i) * 2 + 1] = k1;
    }
}

__global__ void k_knn2_merge(const u32 *__restrict__ part, int na, int nsplit, int32_t *__restrict__ idx,
                             int32_t *__restrict__ dist)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= na) return;
    u32 k0 = 0xFFFFFFFFu, k1 = 0xFFFFFFFFu;
    for (int s = 0; s < nsplit; ++s)
        for (int e = 0; e < 2; ++e) {
            const u32 key = part[((size_t)s * na + i) * 2 + e];
            const u32 m = umax(k0, key);
            k0 = umin(k0, key);
            k1 = umin(k1, m);
        }
    idx[2 * i] = k0 == 0xFFFFFFFFu ? -1 : (int32_t)(k0 & 0x3FFFFFu);
    dist[2 * i] = k0 == 0xFFFFFFFFu ? -1 : (int32_t)(k0 >> 22);
    idx[2 * i + 1] = k1 == 0xFFFFFFFFu ? -1 : (int32_t)(k1 & 0x3FFFFFu);
    dist[2 * i + 1] = k1 == 0xFFFFFFFFu ? -1 : (int32_t)(k1 >> 22);
}

// ---------------------------------------------------------------------------------------------
// All-pairs u16 distance matrix.  Each lane keeps 8 consecutive B rows (64 VGPRs); A rows stream
// through the scalar cache; per A row a lane produces 8 distances packed into one 16-byte store,
// so a wave writes 1 KiB of one output row per instruction (HBM-write-bound shape).
// grid.x = column tiles of 2048 (4 waves x 64 lanes x 8), grid.y = row tiles of MAT_ROWS.
constexpr int MAT_ROWS = 128;      // row tile of the unaligned fallback kernel
constexpr int MAT_UNIT_ROWS = 8;   // rows per work unit of the persistent kernel

// Persistent: the grid is sized to what is resident at once (a grid a few percent larger than that
// runs a second, almost empty round and loses ~30 %).  A workgroup is bound to one column tile
// (blockIdx % n_col_tiles) so its 8 x 256 B columns stay in registers, and takes the 8-row units
// k, k + K, k + 2K, ... of that tile (K = workgroups per column tile): no atomics, no barriers.
// FULL = every lane's 8 columns exist (all column tiles except possibly the last).
template <bool FULL>
__device__ __forceinline__ void matrix_body(const uint4 *__restrict__ A, int64_t na, const uint4 *__restrict__ B, int64_t nb,
                                            uint16_t *__restrict__ out, int ct, int k0, int kstep, int n_units)
{
    const int64_t j0 = ((int64_t)ct * 256 + threadIdx.x) * 8;
    u32 b[8][8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int64_t j = FULL || j0 + c < nb ? j0 + c : nb - 1;
        const uint4 lo = B[2 * j], hi = B[2 * j + 1];
        b[c][0] = lo.x; b[c][1] = lo.y; b[c][2] = lo.z; b[c][3] = lo.w;
        b[c][4] = hi.x; b[c][5] = hi.y; b[c][6] = hi.z; b[c][7] = hi.w;
    }
    if (!FULL && j0 >= nb) return;
    // A rows come through the scalar cache, one fetch in flight: the fetch of the next row (of this unit,
    // or the first row of this workgroup's next unit) is issued as soon as the current row has landed and
    // hides behind the current row's ~135 VALU instructions (see srow_landed).
    // Measured r2 (tools/exp_matrix2.hip, interleaved rounds on one MI355X, 20000 x 20000): the r1 form of this loop
    // 218 us; non-temporal stores (the 800 MB output is written once and never read here: nt keeps it from evicting the
    // B rows' lines and its store stream alone runs 6.3 instead of 5.7 TB/s) 202 us; the 8 distances of a lane as 8
    // accumulator chains in pinned order (ham8_cols) and 6 resident workgroups per CU 168 us = 0.60 of 8 TB/s, the same
    // loop without its store 160 us: the kernel is bound by the VALU's ~2.5 T pairs/s on this formulation, not by HBM.
    // (After an idle period the chip needs ~40 ms of load before it runs at this rate: bench.py pre-rolls.)
    // row indices are 32-bit (launch_matrix checks na < 2^31): clamps and bound tests stay on the scalar unit
    const int last = (int)na - 1, n_rows = (int)na;
    auto row_at = [&](int i) { return min(i, last); };
    const int i_first = row_at(k0 * MAT_UNIT_ROWS);
    uint4 ra = A[2 * (int64_t)i_first], rb = A[2 * (int64_t)i_first + 1];
    typedef u32 v4u __attribute__((ext_vector_type(4)));
    const u32 lane_off = (u32)(j0 * 2);                                   // byte offset inside an output row: the row base is wave-uniform
    for (int unit = k0; unit < n_units; unit += kstep) {
        const int i0 = unit * MAT_UNIT_ROWS;
        const bool whole = i0 + MAT_UNIT_ROWS <= n_rows;                  // wave-uniform: no per-row bound checks in whole units
#pragma unroll
        for (int e = 0; e < MAT_UNIT_ROWS; ++e) {
            srow_landed(ra.x);
            const int inext = row_at(e + 1 < MAT_UNIT_ROWS ? i0 + e + 1 : i0 + kstep * MAT_UNIT_ROWS);
            const uint4 na_ = A[2 * (int64_t)inext], nb_ = A[2 * (int64_t)inext + 1];
            __builtin_amdgcn_sched_barrier(0);
            const u32 rw[8] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w};
            u32 o[8];
            ham8_cols<8>(b, rw, o);                                       // 8 accumulator chains, order pinned (see ham8_cols)
            u32 w[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) w[p] = o[2 * p] | (o[2 * p + 1] << 16);
            if (whole || i0 + e < n_rows) {
                char *row = reinterpret_cast<char *>(out + (int64_t)(i0 + e) * nb);            // scalar registers
                if (FULL || j0 + 8 <= nb) {
                    // SGPR row base + 32-bit lane offset: no vector address arithmetic per row; non-temporal
                    const v4u v = {w[0], w[1], w[2], w[3]};
                    asm volatile("global_store_dwordx4 %0, %1, %2 nt" ::"v"(lane_off), "v"(v), "s"(row) : "memory");
                } else {
                    uint16_t *o = reinterpret_cast<uint16_t *>(row + lane_off);
                    for (int c = 0; c < 8 && j0 + c < nb; ++c) o[c] = (uint16_t)(w[c >> 1] >> ((c & 1) * 16));
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            ra = na_;
            rb = nb_;
        }
    }
}

__global__ __launch_bounds__(256) void k_hamming_matrix(const uint4 *__restrict__ A, int64_t na,
                                                        const uint4 *__restrict__ B, int64_t nb,
                                                        uint16_t *__restrict__ out, int n_col_tiles, int n_units)
{
    const int ct = blockIdx.x % n_col_tiles;
    const int k0 = blockIdx.x / n_col_tiles, kstep = gridDim.x / n_col_tiles;
    if ((int64_t)(ct + 1) * 2048 <= nb) matrix_body<true>(A, na, B, nb, out, ct, k0, kstep, n_units);
    else matrix_body<false>(A, na, B, nb, out, ct, k0, kstep, n_units);
}

// slow path for outputs whose rows are not 16-byte aligned (nb % 8 != 0)
__global__ void k_hamming_matrix_any(const uint4 *__restrict__ A, int64_t na, const uint4 *__restrict__ B,
                                     int64_t nb, uint16_t *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.y * MAT_ROWS;
    const int64_t i1 = i0 + MAT_ROWS < na ? i0 + MAT_ROWS : na;
    if (j >= nb) return;
    u32 q[8];
    const uint4 lo = B[2 * j], hi = B[2 * j + 1];
    q[0] = lo.x; q[1] = lo.y; q[2] = lo.z; q[3] = lo.w; q[4] = hi.x; q[5] = hi.y; q[6] = hi.z; q[7] = hi.w;
    for (int64_t i = i0; i < i1; ++i) out[i * nb + j] = (uint16_t)ham8(q, A[2 * i], A[2 * i + 1], 0);
}

static int launch_matrix(reloc_ctx *ctx, const uint8_t *a, int64_t na, const uint8_t *b, int64_t nb, uint16_t *out)
{
    if (na <= 0 || nb <= 0) return RELOC_OK;
    if (nb % 8 == 0 && ((uintptr_t)out & 15) == 0) {
        const int n_col_tiles = (int)((nb + 2047) / 2048);
        const int64_t n_units = (na + MAT_UNIT_ROWS - 1) / MAT_UNIT_ROWS;
        if (n_col_tiles > 4096 || na > 0x7ffffff0 || nb * 2 > 0xffffffffll) { reloc_set_error("hamming matrix: shape too large"); return RELOC_E_CAPACITY; }
        static int per_cu = 0;
        if (!per_cu) {
            // blocks of 4 waves = one wave per SIMD each: residency = waves per SIMD the register
            // allocation admits, capped by the occupancy query (which can over-report by one)
            hipFuncAttributes fa;
            int api = 0;
            per_cu = 4;
            if (hipFuncGetAttributes(&fa, (const void *)k_hamming_matrix) == hipSuccess && fa.numRegs > 0) {
                const int alloc = (fa.numRegs + 7) / 8 * 8;
                per_cu = 512 / alloc < 8 ? 512 / alloc : 8;
            }
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&api, k_hamming_matrix, 256, 0) == hipSuccess && api > 0 && api < per_cu)
                per_cu = api;
            if (per_cu > 6) per_cu = 6;           // measured (8 chains): 5 / 6 / 7 resident workgroups per CU 174 / 168 / 189 us
            if (per_cu < 1) per_cu = 1;
        }
        int grid = ctx->num_cu * per_cu;
        grid = grid / n_col_tiles * n_col_tiles;
        if (grid < n_col_tiles) grid = n_col_tiles;
        const int64_t cap = n_units * n_col_tiles;
        if (grid > cap) grid = (int)cap;
        reloc_prof_begin(ctx, RELOC_PROF_MATRIX);
        hipLaunchKernelGGL(k_hamming_matrix, dim3(grid), dim3(256), 0, ctx->stream, (const uint4 *)a, na, (const uint4 *)b, nb,
                           out, n_col_tiles, (int)n_units);
        reloc_prof_end(ctx, RELOC_PROF_MATRIX);
    } else {
        const int64_t gy = (na + MAT_ROWS - 1) / MAT_ROWS;
        if (gy > 65535) { reloc_set_error("hamming matrix: too many rows for the unaligned path"); return RELOC_E_CAPACITY; }
        reloc_prof_begin(ctx, RELOC_PROF_MATRIX);
        dim3 grid((unsigned)((nb + 255) / 256), (unsigned)gy);
        hipLaunchKernelGGL(k_hamming_matrix_any, grid, dim3(256), 0, ctx->stream, (const uint4 *)a, na, (const uint4 *)b, nb, out);
        reloc_prof_end(ctx, RELOC_PROF_MATRIX);
    }
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}

// ---------------------------------------------------------------------------------------------
// C-ABI entry points
RELOC_API int reloc_hamming_matrix_dev(reloc_ctx *ctx, const uint8_t *a, int64_t na, const uint8_t *b, int64_t nb,
                                       uint16_t *out)
{
    ARG_CHECK_CTX(ctx, a && b && out && na >= 0 && nb >= 0, "reloc_hamming_matrix_dev");
    ARG_CHECK((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "descriptor arrays must be 16-byte aligned");
    return launch_matrix(ctx, a, na, b, nb, out);
}

RELOC_API int reloc_hamming_matrix(reloc_ctx *ctx, const uint8_t *a, int64_t na, const uint8_t *b, int64_t nb,
                                   uint16_t *out)
{
    ARG_CHECK_CTX(ctx, a && b && out && na >= 0 && nb >= 0, "reloc_hamming_matrix");
    if (na == 0 || nb == 0) return RELOC_OK;
    HostStaging st{ctx};
    const uint8_t *da = st.upload_slot(0, a, na * 32), *db = st.upload_slot(1, b, nb * 32);
    uint16_t *dout = st.slot<uint16_t>(2, na * nb);
    st.run([&] { return launch_matrix(ctx, da, na, db, nb, dout); });
    st.download(out, dout, na * nb * 2);
    return st.finish();
}

RELOC_API int reloc_match_knn2(reloc_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int32_t *idx,
                               int32_t *dist)
{
    ARG_CHECK_CTX(ctx, nq >= 0 && nt >= 0 && (nq == 0 || (q && idx && dist)) && (nt == 0 || t), "reloc_match_knn2");
    if (nq == 0) return RELOC_OK;
    if (nt == 0) {
        for (int i = 0; i < 2 * nq; ++i) { idx[i] = -1; dist[i] = -1; }
        return RELOC_OK;
    }
    if (nt >= (1 << 22)) { reloc_set_error("knn2: train set too large"); return RELOC_E_CAPACITY; }
    int nsplit = (int)((int64_t)ctx->num_cu * 4 / ((nq + 255) / 256));
    if (nsplit < 1) nsplit = 1;
    if (nsplit > (nt + 63) / 64) nsplit = (nt + 63) / 64;
    const int rows_per_split = (nt + nsplit - 1) / nsplit;
    nsplit = (nt + rows_per_split - 1) / rows_per_split;
    HostStaging st{ctx};
    u32 *dpart = st.slot<u32>(2, (int64_t)nsplit * nq * 2);
    int32_t *didx = st.slot<int32_t>(3, (int64_t)nq * 4);
    if (st.rc) return st.rc;
    int32_t *ddist = didx + 2 * (size_t)nq;
    const uint8_t *dq = st.upload_slot(0, q, (int64_t)nq * 32), *dt = st.upload_slot(1, t, (int64_t)nt * 32);
    st.launch(k_knn2, dim3((nq + 255) / 256, nsplit), dim3(256), (const uint4 *)dq, nq, (const uint4 *)dt, nt, rows_per_split, dpart);
    st.launch(k_knn2_merge, dim3((nq + 255) / 256), dim3(256), dpart, nq, nsplit, didx, ddist);
    st.download(idx, didx, (int64_t)nq * 8);
    st.download(dist, ddist, (int64_t)nq * 8);
    return st.finish();
}

RELOC_API int reloc_match_mutual(reloc_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int32_t *qidx,
                                 int32_t *tidx, int32_t *dist, int32_t *n_out)
{
    ARG_CHECK_CTX(ctx, n_out && nq >= 0 && nt >= 0, "reloc_match_mutual");
    *n_out = 0;
    if (nq == 0 || nt == 0) return RELOC_OK;
    ARG_CHECK(q && t && qidx && tidx && dist, "reloc_match_mutual: NULL array");
    if (nq > MAX_REC_ROWS) { reloc_set_error("match: query set larger than %d rows", MAX_REC_ROWS); return RELOC_E_CAPACITY; }
    HostStaging st{ctx};
    uint8_t *dq = st.slot<uint8_t>(0, (int64_t)nq * 32 + 64), *dt = st.slot<uint8_t>(1, (int64_t)nt * 32);
    int64_t *doff = (int64_t *)st.slot_bytes(2, (int64_t)nq * 12 + 64);
    if (st.rc) return st.rc;
    // offsets {0, nq} live in front of the match arrays
    const int64_t offs[2] = {0, nq};
    int32_t *dn = (int32_t *)(doff + 2);
    int32_t *dqi = dn + 4, *dti = dqi + nq, *ddi = dti + nq;
    st.upload(doff, offs, sizeof(offs));
    st.upload(dq, q, (int64_t)nq * 32);
    st.upload(dt, t, (int64_t)nt * 32);
    // the query set is the one record (rows nq) of a database of its own; nothing runs beside it: 8 waves
    EmitBatch bt = {};
    bt.f[0].cur = (const uint4 *)dt; bt.f[0].m_qidx = dqi; bt.f[0].m_tidx = dti; bt.f[0].m_dist = ddi; bt.f[0].m_n = dn;
    st.run([&] { return launch_db_emit(&ctx, 1, bt, dq, doff, nq, nullptr, 1, nt, nq, true); });
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
    HostStaging st{ctx};
    uint8_t *dq = st.slot<uint8_t>(0, (int64_t)nq * 32), *dt = st.slot<uint8_t>(1, (int64_t)nt * 32);
    int64_t *doff = (int64_t *)st.slot_bytes(2, (int64_t)nq * 12 + 64);
    if (st.rc) return st.rc;
    // offsets {0, nt} live in front of the list length and the match arrays
    const int64_t offs[2] = {0, nt};
    int32_t *dn = (int32_t *)(doff + 2);
    int32_t *dqi = dn + 4, *dti = dqi + nq, *ddi = dti + nq;
    st.upload(doff, offs, sizeof(offs));
    st.upload(dq, q, (int64_t)nq * 32);
    st.upload(dt, t, (int64_t)nt * 32);
    EmitBatch bt = {};
    bt.f[0].cur = (const uint4 *)dq; bt.f[0].m_qidx = dqi; bt.f[0].m_tidx = dti; bt.f[0].m_dist = ddi; bt.f[0].m_n = dn;
    st.run([&] { return launch_db_ratio_emit(&ctx, 1, bt, dt, doff, nullptr, 1, nq, nq, ratio, 0, 0, true); });
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

// ---- scans of the selected database (the database itself: reloc_db.hip) -----------------------
RELOC_API int reloc_db_match_counts_dev(reloc_ctx *ctx, const uint8_t *cur_dev, const int32_t *n_cur_dev, int n_cur_max,
                                        int32_t *counts_dev)
{
    ARG_CHECK_CTX(ctx, cur_dev && counts_dev && n_cur_max >= 0, "reloc_db_match_counts_dev");
    if (!db_ready(ctx)) { reloc_set_error("no database uploaded"); return RELOC_E_STATE; }
    reloc_prof_begin(ctx, RELOC_PROF_DB_SCAN);
    int rc = launch_db_count(ctx, cur_dev, n_cur_dev, n_cur_max, counts_dev);
    reloc_prof_end(ctx, RELOC_PROF_DB_SCAN);

    return rc;
}

RELOC_API int reloc_db_ratio_counts(reloc_ctx *ctx, const uint8_t *cur, int n_cur, double ratio, int32_t *counts)
{
    ARG_CHECK_CTX(ctx, counts && n_cur >= 0 && (n_cur == 0 || cur) && ratio > 0, "reloc_db_ratio_counts");
    if (!db_ready(ctx)) { reloc_set_error("no database uploaded"); return RELOC_E_STATE; }
    const DbArena &db = ctx_db(ctx);
    if (n_cur == 0) { memset(counts, 0, (size_t)db.records * 4); return RELOC_OK; }
    if (n_cur > 65535) { reloc_set_error("ratio scan: more than 65535 current descriptors"); return RELOC_E_CAPACITY; }
    HostStaging st{ctx};
    const uint8_t *dc = st.upload_slot(0, cur, (int64_t)n_cur * 32);
    int grid = ctx->num_cu * 4;
    if (grid > db.records) grid = (int)db.records;
    st.launch(k_db_ratio<false>, dim3(grid), dim3(256), (const uint4 *)db.desc, db.off, (int)db.records, (const uint4 *)dc,
              (const int32_t *)nullptr, n_cur, ratio, db.counts, ScanMask{}, 0);
    st.download(counts, db.counts, db.records * 4);
    return st.finish();
}

RELOC_API int reloc_db_match_counts(reloc_ctx *ctx, const uint8_t *cur, int n_cur, int32_t *counts)
{
    ARG_CHECK_CTX(ctx, counts && n_cur >= 0 && (n_cur == 0 || cur), "reloc_db_match_counts");
    if (!db_ready(ctx)) { reloc_set_error("no database uploaded"); return RELOC_E_STATE; }
    const DbArena &db = ctx_db(ctx);
    if (n_cur == 0) { memset(counts, 0, (size_t)db.records * 4); return RELOC_OK; }
    HostStaging st{ctx};
    const uint8_t *dc = st.upload_slot(0, cur, (int64_t)n_cur * 32);
    st.run([&] { return reloc_db_match_counts_dev(ctx, dc, nullptr, n_cur, db.counts); });
    st.download(counts, db.counts, db.records * 4);
    return st.finish();
}
