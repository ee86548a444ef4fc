// reloc_scan.hip -- the crossCheck scans of the database on gfx950 (CDNA4): per record the mutual nearest neighbours of its
// teach rows and the current descriptors, counted (k_db_scan, k_db_scan_batch) or listed (k_db_scan_emit, k_db_scan_emit_batch).
//
// Serves cv2.BFMatcher(NORM_HAMMING, crossCheck=True).match        (reference M:211,327; G:337)
//        the whole-database candidate scoring of variant G          (reference G:329-344)
// The file holds those kernels, their launchers and the entry points that run them (reloc_match_mutual,
// reloc_db_match_counts*); the few-query count is in reloc_scan_rows.hip, the Lowe-ratio policy in reloc_ratio.hip, the
// primitives and their measured instruction costs in reloc_hamming.h; the database they scan is kept by reloc_db.hip.
//
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
#include "reloc_hamming.h"

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
    const int C = cur_count(n_cur_p, n_cur_max);
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
    const int C = cur_count(n_cur_p, n_cur_max);
    db_emit_body<NJ, NW>(lds, C, db, off, rec_ids, n_ids_p, n_ids_max, cur, max_rows, m_qidx, m_tidx, m_dist, m_n, emit_stride, g_pts3d,
                         g_xy, g_obj, g_img);
}

// The emit pass (match lists of the candidate records, M:327-336) of up to 8 frames in one launch: blockIdx.y = frame.
__global__ __launch_bounds__(256, 4) RELOC_SCAN_VGPR_ATTR void k_db_scan_emit_batch(const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_ids_max,
                                                          int n_cur_max, int max_rows, int emit_stride, const float *__restrict__ g_pts3d,
                                                          EmitBatch bt)
{
    extern __shared__ u32 lds[];
    RELOC_SMALL_KERNEL_PRIO();
    const EmitFrame &F = bt.f[blockIdx.y];
    const int C = cur_count(F.n_cur_p, n_cur_max);
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

// the counting scans of up to 8 frames in one launch: workgroup b scans frame b % bt.n (ScanBatch, reloc_hamming.h)
__global__ __launch_bounds__(256, 4) RELOC_SCAN_VGPR_ATTR void k_db_scan_batch(const uint4 *__restrict__ db, const int64_t *__restrict__ off, int n_ids,
                                                          int n_cur_max, int max_rows, ScanBatch bt, u32 *ticket_pool, int quota, int n_bounded, int col_words)
{
    extern __shared__ u32 lds[];
    const int f = blockIdx.x % bt.n;                       // workgroup-uniform
    const ScanMask mask = scan_mask_of(bt, f);
    const int C = cur_count(bt.n_cur[f], n_cur_max);
    db_count_body<8>(lds, C, db, off, nullptr, nullptr, n_ids, bt.cur[f], max_rows, bt.counts[f], mask, ticket_pool + f * 8 * TICKET_STRIDE, quota,
                     n_bounded, col_words, ticket_pool, bt.n, (int)(blockIdx.x / bt.n), (int)((gridDim.x + bt.n - 1 - f) / bt.n));
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
    if (int rc = ctx->scan_block.layout(ctx, [&](BlockCarver &c) { c.own(ctx->scan_ticket, SCAN_TICKET_WORDS); })) return rc;
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
    if (int rc = scan_capacity_check("db scan", n_cur_max, db.max_rows)) return rc;
    const int max_rows = db.max_rows < 1 ? 1 : db.max_rows;
    const uint4 *desc = (const uint4 *)db.desc;
    if (!mask.xyh && n_cur_max <= 64 && max_rows <= SQ_MAX_ROWS)       // few queries: lane = teach row (reloc_scan_rows.hip)
        return launch_db_count_rows(ctx, desc, db.off, n_ids, cur, n_cur_dev, n_cur_max, counts);
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
    if (int rc = scan_capacity_check("db scan", n_cur_max, max_rows)) return rc;
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
    const ScanBatch bt = scan_batch(ctxs, n, auto_mode, heading_mask ? db.xy_heading : nullptr, cos_tol, [&](int g) { return q + 4 * g; });
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

// ---------------------------------------------------------------------------------------------
// C-ABI entry points
RELOC_API int reloc_match_mutual(reloc_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int32_t *qidx,
                                 int32_t *tidx, int32_t *dist, int32_t *n_out)
{
    ARG_CHECK_CTX(ctx, n_out && nq >= 0 && nt >= 0, "reloc_match_mutual");
    *n_out = 0;
    if (nq == 0 || nt == 0) return RELOC_OK;
    ARG_CHECK(q && t && qidx && tidx && dist, "reloc_match_mutual: NULL array");
    if (nq > MAX_REC_ROWS) { reloc_set_error("match: query set larger than %d rows", MAX_REC_ROWS); return RELOC_E_CAPACITY; }
    // the query set is the one record (rows nq, its buffer 64 bytes longer) of a database of its own; nothing runs beside it: 8 waves
    return match_one_record(ctx, q, nq, 64, t, nt, true, qidx, tidx, dist, n_out, [&](const EmitBatch &bt, const uint8_t *rec, const int64_t *off) {
        return launch_db_emit(&ctx, 1, bt, rec, off, nq, nullptr, 1, nt, nq, true);
    });
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
