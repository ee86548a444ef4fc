// reloc_scan_rows.hip -- the whole-database crossCheck count for few current descriptors: k_db_scan_rows, a lane per teach row,
// and its launcher.  launch_db_count (reloc_scan.hip) decides when it runs; the primitives it shares: reloc_hamming.h.
#include "reloc_hamming.h"

// ---------------------------------------------------------------------------------------------
// Few current descriptors (C <= 64): the roles swap.  With one or a few dozen queries the column-per-lane kernel
// above wastes its 128 lanes x columns (Q = 1 and Q = 32 both cost the 128-column price, 55 us at 10 000 x 64); here a
// LANE is a teach row -- the wave reads 64 rows of the record straight from HBM (2 KB, coalesced), the queries are
// wave-uniform and arrive through the scalar cache -- so the work follows C and the kernel runs at the pace of the
// database read up to Q ~ 8.  One wave owns a record (no barriers); the SIMD's eight waves hide each other's HBM latency
// (one record per wave turn: taking two or four per turn lets the SIMD's waves fall into step, profiles/r3_small_q_records_per_turn.log).
// Records of more than SQ_MAX_ROWS rows (reloc_hamming.h), emit mode and the heading mask stay with k_db_scan.
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
                     "v_permlane16_swap_b32 %0, %4\n\t"              // %0, %4 were last written 7 and 5 instructions ago
                     SQ_NOP                                          // %12 was written by the instruction in front of that swap,
                     "v_permlane16_swap_b32 %8, %12\n\t"             // which is one wait state of the two: pad
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
    const int C = cur_count(n_cur_p, n_cur_max);
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

// few queries: lane = teach row (k_db_scan_rows)
int launch_db_count_rows(reloc_ctx *ctx, const uint4 *desc, const int64_t *off, int n_ids, const uint8_t *cur, const int32_t *n_cur_dev,
                         int n_cur_max, int32_t *counts)
{
    if (n_cur_max == 0) {                              // a capacity of zero descriptors: nothing may be read from `cur`
        HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_ids * sizeof(int32_t), ctx->stream));
        return RELOC_OK;
    }
    int grid = ctx->num_cu * 8;                        // 8 workgroups of 4 waves per CU
    const int need = (n_ids + SQ_WAVES - 1) / SQ_WAVES;
    if (grid > need) grid = need;
#define RELOC_LAUNCH_ROWS(G, HOIST)                                                                                           \
    hipLaunchKernelGGL((k_db_scan_rows<G, HOIST>), dim3(grid), dim3(64 * SQ_WAVES), 0, ctx->stream, desc, off, n_ids, \
                       (const uint4 *)cur, n_cur_dev, n_cur_max, counts)
    // G = queries per butterfly group: a call with 1-4 queries evaluates 4 distances per row, not 16; its query words stay in SGPRs
    if (n_cur_max <= 4) RELOC_LAUNCH_ROWS(4, true); else if (n_cur_max <= 8) RELOC_LAUNCH_ROWS(8, false); else RELOC_LAUNCH_ROWS(16, false);
#undef RELOC_LAUNCH_ROWS
    HIP_TRY(hipGetLastError());
    return RELOC_OK;
}
