// Developer microbenchmark: issue cost of the f32-denormal argmin keys of k_db_scan on gfx950, in real shader cycles
// (same clock and stream shape as tools/ubench_valu2.hip).
//   hipcc --offload-arch=gfx950 -O3 -o tools/ubench_fkey tools/ubench_fkey.hip && ./tools/ubench_fkey
// A key d << 7 | idx (< 2^16) read as an f32 is a positive denormal, so fma(d, 128.0f, idx) builds it exactly and the
// f32 minima order it like the integer.  Measured: v_fmaak_f32 / v_fma_f32 on denormal operands, v_min3_f32 / v_min_f32
// on denormal keys, and one teach row of the scan (8 columns: 64 xor + 64 bcnt + bookkeeping): the shift + or key, the
// FMA key with a min3_f32 row tree, the FMA key with the v_min_u16 row tree (the form k_db_scan uses).
// Every operand stays a denormal: the FMAs write fresh registers from loop-invariant distances <= 255.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#define ITERS 2048

template <int MODE>
__global__ __launch_bounds__(256) void k(uint32_t *out, uint64_t *stamps, uint32_t seed)
{
    uint32_t a0 = (threadIdx.x + seed) & 255u, a1 = (a0 * 3) & 255u, a2 = (a0 * 5) & 255u, a3 = (a0 * 7) & 255u;
    uint32_t a4 = (a0 * 11) & 255u, a5 = (a0 * 13) & 255u, a6 = (a0 * 17) & 255u, a7 = (a0 * 19) & 255u;
    uint32_t b0 = a0 << 7, b1 = a1 << 7, b2 = a2 << 7, b3 = a3 << 7, b4 = a4 << 7, b5 = a5 << 7, b6 = a6 << 7, b7 = a7 << 7;
    uint32_t c128 = 0x43000000u, ck = 0x45u;   // 128.0f; an index as a denormal
    asm volatile("" : "+v"(c128), "+v"(ck));
    const uint32_t s = __builtin_amdgcn_readfirstlane(seed * 2654435761u);
    const uint64_t t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < ITERS; ++i) {
#define V2(INS, d, x) asm volatile(INS " %0, %0, %1" : "+v"(d) : "v"(x));
#define V3(INS, d, x) asm volatile(INS " %0, %0, %1, %2" : "+v"(d) : "v"(x), "v"(b7));
#define FK(INS, d, x) asm volatile("v_fmaak_f32 %0, %1, %2, 0x45" : "=v"(d) : "v"(x), "v"(c128));
#define FV(INS, d, x) asm volatile("v_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(x), "v"(c128), "v"(ck));
#define REP16(M, INS) M(INS, a0, a1) M(INS, a1, a2) M(INS, a2, a3) M(INS, a3, a4) M(INS, a4, a5) M(INS, a5, a6) M(INS, a6, a7) M(INS, a7, a0) \
                      M(INS, a0, a1) M(INS, a1, a2) M(INS, a2, a3) M(INS, a3, a4) M(INS, a4, a5) M(INS, a5, a6) M(INS, a6, a7) M(INS, a7, a0)
#define REP16B(M, INS) M(INS, b0, a0) M(INS, b1, a1) M(INS, b2, a2) M(INS, b3, a3) M(INS, b4, a4) M(INS, b5, a5) M(INS, b6, a6) M(INS, b7, a7) \
                       M(INS, b0, a1) M(INS, b1, a2) M(INS, b2, a3) M(INS, b3, a4) M(INS, b4, a5) M(INS, b5, a6) M(INS, b6, a7) M(INS, b7, a0)
        if (MODE == 0) { REP16(V2, "v_xor_b32") }
        if (MODE == 1) { REP16(V2, "v_min_u16") }
        if (MODE == 2) { REP16B(FK, "") }
        if (MODE == 3) { REP16B(FV, "") }
        if (MODE == 4) { REP16(V3, "v_min3_f32") }
        if (MODE == 5) { REP16(V2, "v_min_f32") }
        if (MODE == 6) { REP16(V3, "v_min3_u32") }
        if (MODE == 7) {   // the old key: v_lshlrev_b16 + v_or_b32 (8 keys, 16 instructions)
#define OK(d, x) asm volatile("v_lshlrev_b16 %0, 7, %1" : "=v"(d) : "v"(x)); asm volatile("v_or_b32 %0, 0x45, %0" : "+v"(d));
            OK(b0, a0) OK(b1, a1) OK(b2, a2) OK(b3, a3) OK(b4, a4) OK(b5, a5) OK(b6, a6) OK(b7, a7)
        }
        if (MODE >= 8 && MODE <= 10) {  // one teach row against 8 columns, as scan_chunk emits it (8: 8 shl + 8 or + 8 + 7
                                        // v_min_u16; 9: 8 v_fmaak_f32 + 8 v_min_u16 + 3 v_min3_f32 + v_min_f32;
                                        // 10: 8 v_fmaak_f32 + 8 + 7 v_min_u16)
            const uint32_t q[8] = {a0, a1, a2, a3, a4, a5, a6, a7};
            uint32_t cb[8] = {b0, b1, b2, b3, b4, b5, b6, b7}, h[8];
#pragma unroll
            for (int w = 0; w < 8; ++w)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    uint32_t x;
                    asm volatile("v_xor_b32 %0, %1, %2" : "=v"(x) : "s"(s), "v"(q[j]));
                    if (w == 0) asm volatile("v_bcnt_u32_b32 %0, %1, 0" : "=v"(h[j]) : "v"(x));
                    else asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(h[j]) : "v"(x));
                }
            uint32_t best;
            if (MODE == 8) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    asm volatile("v_lshlrev_b16 %0, 7, %0" : "+v"(h[j]));
                    asm volatile("v_or_b32 %0, %1, %0" : "+v"(h[j]) : "n"(0x40 + j));
                    asm volatile("v_min_u16 %0, %0, %1" : "+v"(cb[j]) : "v"(h[j]));
                }
#pragma unroll
                for (int j = 0; j < 8; j += 2) asm volatile("v_min_u16 %0, %0, %1" : "+v"(h[j]) : "v"(h[j + 1]));
                asm volatile("v_min_u16 %0, %0, %1" : "+v"(h[0]) : "v"(h[2]));
                asm volatile("v_min_u16 %0, %0, %1" : "+v"(h[4]) : "v"(h[6]));
                asm volatile("v_min_u16 %0, %0, %1" : "+v"(h[0]) : "v"(h[4]));
                best = h[0];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    asm volatile("v_fmaak_f32 %0, %0, %1, %2" : "+v"(h[j]) : "v"(c128), "n"(0x40 + j));
                    asm volatile("v_min_u16 %0, %0, %1" : "+v"(cb[j]) : "v"(h[j]));
                }
            }
            if (MODE == 10) {
#pragma unroll
                for (int j = 0; j < 8; j += 2) asm volatile("v_min_u16 %0, %0, %1" : "+v"(h[j]) : "v"(h[j + 1]));
                asm volatile("v_min_u16 %0, %0, %1" : "+v"(h[0]) : "v"(h[2]));
                asm volatile("v_min_u16 %0, %0, %1" : "+v"(h[4]) : "v"(h[6]));
                asm volatile("v_min_u16 %0, %0, %1" : "+v"(h[0]) : "v"(h[4]));
                best = h[0];
            } else if (MODE == 9) {
                asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(h[0]) : "v"(h[1]), "v"(h[2]));
                asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(h[3]) : "v"(h[4]), "v"(h[5]));
                asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(h[0]) : "v"(h[3]), "v"(h[6]));
                asm volatile("v_min_f32 %0, %0, %1" : "+v"(h[0]) : "v"(h[7]));
                best = h[0];
            }
            b0 = cb[0]; b1 = cb[1]; b2 = cb[2]; b3 = cb[3]; b4 = cb[4]; b5 = cb[5]; b6 = cb[6]; b7 = cb[7] ^ (best >> 15);
        }
    }
    const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7 ^ b0 ^ b1 ^ b2 ^ b3 ^ b4 ^ b5 ^ b6 ^ b7;
    if (threadIdx.x == 0) { stamps[2 * blockIdx.x] = t1 - t0; stamps[2 * blockIdx.x + 1] = r1 - r0; }
}

static uint32_t *d_out; static uint64_t *d_st;

template <int MODE> void run(const char *name, int per_cu, double instr_per_iter, double pairs_per_iter = 0)
{
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    const int grid = 256 * per_cu;
    for (int r = 0; r < 3; ++r) hipLaunchKernelGGL(k<MODE>, dim3(grid), dim3(256), 0, 0, d_out, d_st, 1u);
    hipDeviceSynchronize();
    hipEventRecord(a);
    const int reps = 10;
    for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k<MODE>, dim3(grid), dim3(256), 0, 0, d_out, d_st, 1u);
    hipEventRecord(b); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b); ms /= reps;
    std::vector<uint64_t> st(2 * grid);
    hipMemcpy(st.data(), d_st, st.size() * 8, hipMemcpyDeviceToHost);
    std::vector<double> clk, cyc;
    for (int i = 0; i < grid; ++i) { clk.push_back((double)st[2 * i] / (double)st[2 * i + 1] * 100e6); cyc.push_back((double)st[2 * i]); }
    std::sort(clk.begin(), clk.end()); std::sort(cyc.begin(), cyc.end());
    const double f = clk[grid / 2], wave_cycles = cyc[grid / 2];
    const double winstr = (double)ITERS * instr_per_iter;                  // per wave
    const double cyc_per_instr = wave_cycles / (winstr * per_cu);          // cycles per wave-instruction per SIMD
    printf("%-34s waves/SIMD=%d  clock %.2f GHz  %.2f real cyc/wave-instr/SIMD  %.1f real cyc/iter/SIMD", name, per_cu, f / 1e9,
           cyc_per_instr, wave_cycles / ((double)ITERS * per_cu));
    if (pairs_per_iter > 0) printf("  %.2f T pairs/s", (double)grid * 256 * ITERS * pairs_per_iter / (ms * 1e-3) / 1e12);
    printf("\n");
    fflush(stdout);
}

int main()
{
    hipMalloc(&d_out, 256 * 8 * 256 * 4); hipMalloc(&d_st, 256 * 8 * 16);
    for (int w : {4, 8}) {
        run<0>("v_xor_b32 v,v", w, 16); run<1>("v_min_u16", w, 16);
        run<2>("v_fmaak_f32 (denormal)", w, 16); run<3>("v_fma_f32 (denormal)", w, 16);
        run<4>("v_min3_f32 (denormal)", w, 16); run<5>("v_min_f32 (denormal)", w, 16); run<6>("v_min3_u32", w, 16);
        run<7>("old key: lshlrev_b16 + or", w, 16);
        run<8>("scan row old: +8 shl +8 or +15 min16", w, 64 + 64 + 31, 8);
        run<9>("scan row: +8 fmaak +8 min16 +4 fmin", w, 64 + 64 + 20, 8);
        run<10>("scan row: +8 fmaak +15 min16", w, 64 + 64 + 23, 8);
    }
    return 0;
}
