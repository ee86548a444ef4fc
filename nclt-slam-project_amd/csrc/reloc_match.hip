// reloc_match.hip -- the two generic 256-bit Hamming matchers on gfx950 (CDNA4), XOR + popcount on the VALU.
//
// Serves cv2.BFMatcher(NORM_HAMMING, crossCheck=False).knnMatch k=2 (reference S:46,68)
// and the all-pairs u16 distance matrix of BASELINE.json config 5.
// The file holds those kernels, the matrix launcher and their entry points (reloc_match_knn2, reloc_hamming_matrix*).  The
// scans of a database are in reloc_scan.hip (crossCheck), reloc_scan_rows.hip (its few-query count) and reloc_ratio.hip (Lowe
// ratio); the primitives all four share, with their measured instruction costs, in reloc_hamming.h.
#include "reloc_hamming.h"

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
