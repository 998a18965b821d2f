// valu_rate_trans.hip -- microbenchmark (not product), sibling of valu_rate.hip: issue cost on gfx950 of the instructions that
// re-normalising a unit vector is made of -- the transcendentals (v_rcp_f32, v_rsq_f32, v_sqrt_f32), fp64 multiplies and
// fp32 <-> fp64 conversions (pow32), and an LDS read with a per-lane address among 16 consecutive dwords (the table of
// rtx_unit.hpp) -- and of the two whole sequences: rsq + rcp with their correction steps against subtract, mask, shift, read.
// Same form as valu_rate.hip: every wave runs ITERS iterations of 8 independent chains; cycles per wave-instruction (or per
// sequence) and SIMD with 1, 2, 4, 8 waves per SIMD resident.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o valu_rate_trans valu_rate_trans.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
constexpr int ITERS = 4096;

#define OP8_1(TXT) asm volatile(TXT " %0, %0\n\t" TXT " %1, %1\n\t" TXT " %2, %2\n\t" TXT " %3, %3\n\t" \
                                TXT " %4, %4\n\t" TXT " %5, %5\n\t" TXT " %6, %6\n\t" TXT " %7, %7" \
                                : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7))

template <int KIND> __global__ void k(float* out, float seed)
{
    __shared__ uint32_t s_tab[16];
    const float a = seed + (float)(threadIdx.x & 7) * 0.125f, b = 1.0001f;
    float x0 = a + 1, x1 = a + 2, x2 = a + 3, x3 = a + 4, x4 = a + 5, x5 = a + 6, x6 = a + 7, x7 = a + 8;
    if (KIND == 0) { // v_mul_f32: the plain instruction everything is set against
        for (int i = 0; i < ITERS; i++) {
            asm volatile("v_mul_f32 %0, %0, %8\n\tv_mul_f32 %1, %1, %8\n\tv_mul_f32 %2, %2, %8\n\tv_mul_f32 %3, %3, %8\n\t"
                         "v_mul_f32 %4, %4, %8\n\tv_mul_f32 %5, %5, %8\n\tv_mul_f32 %6, %6, %8\n\tv_mul_f32 %7, %7, %8"
                         : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(b));
        }
    } else if (KIND == 1) {
        for (int i = 0; i < ITERS; i++) OP8_1("v_rcp_f32");
    } else if (KIND == 2) {
        for (int i = 0; i < ITERS; i++) OP8_1("v_rsq_f32");
    } else if (KIND == 3) {
        for (int i = 0; i < ITERS; i++) OP8_1("v_sqrt_f32");
    } else if (KIND == 4) { // v_mul_f64 (pow32's squarings)
        double d0 = x0, d1 = x1, d2 = x2, d3 = x3, d4 = x4, d5 = x5, d6 = x6, d7 = x7;
        const double bd = 1.0000001;
        for (int i = 0; i < ITERS; i++) {
            asm volatile("v_mul_f64 %0, %0, %8\n\tv_mul_f64 %1, %1, %8\n\tv_mul_f64 %2, %2, %8\n\tv_mul_f64 %3, %3, %8\n\t"
                         "v_mul_f64 %4, %4, %8\n\tv_mul_f64 %5, %5, %8\n\tv_mul_f64 %6, %6, %8\n\tv_mul_f64 %7, %7, %8"
                         : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3), "+v"(d4), "+v"(d5), "+v"(d6), "+v"(d7) : "v"(bd));
        }
        x0 = (float)(d0 + d1 + d2 + d3); x1 = (float)(d4 + d5 + d6 + d7);
    } else if (KIND == 5) { // v_cvt_f64_f32 / v_cvt_f32_f64 alternating (16 instructions per iteration)
        for (int i = 0; i < ITERS / 2; i++) {
            double t0, t1, t2, t3, t4, t5, t6, t7;
            asm volatile("v_cvt_f64_f32 %8, %0\n\tv_cvt_f64_f32 %9, %1\n\tv_cvt_f64_f32 %10, %2\n\tv_cvt_f64_f32 %11, %3\n\t"
                         "v_cvt_f64_f32 %12, %4\n\tv_cvt_f64_f32 %13, %5\n\tv_cvt_f64_f32 %14, %6\n\tv_cvt_f64_f32 %15, %7\n\t"
                         "v_cvt_f32_f64 %0, %8\n\tv_cvt_f32_f64 %1, %9\n\tv_cvt_f32_f64 %2, %10\n\tv_cvt_f32_f64 %3, %11\n\t"
                         "v_cvt_f32_f64 %4, %12\n\tv_cvt_f32_f64 %5, %13\n\tv_cvt_f32_f64 %6, %14\n\tv_cvt_f32_f64 %7, %15"
                         : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7), "=&v"(t0), "=&v"(t1), "=&v"(t2),
                           "=&v"(t3), "=&v"(t4), "=&v"(t5), "=&v"(t6), "=&v"(t7));
        }
    } else if (KIND == 6) { // ds_read_b32, per-lane address among 16 consecutive dwords; each read's result is the next address
        const uint32_t base = (uint32_t)(size_t)(__attribute__((address_space(3))) void*)s_tab; // LDS byte address of the table
        if (threadIdx.x < 16) s_tab[threadIdx.x] = base + 4u * ((threadIdx.x * 5u + 3u) & 15u); // byte addresses, a 16-cycle permutation
        __syncthreads();
        const uint32_t t = threadIdx.x;
        uint32_t u0 = base + 4u * (t & 15u), u1 = base + 4u * ((t + 1u) & 15u), u2 = base + 4u * ((t + 2u) & 15u), u3 = base + 4u * ((t + 3u) & 15u);
        uint32_t u4 = base + 4u * ((t + 4u) & 15u), u5 = base + 4u * ((t + 5u) & 15u), u6 = base + 4u * ((t + 6u) & 15u), u7 = base + 4u * ((t + 7u) & 15u);
        for (int i = 0; i < ITERS; i++) {
            asm volatile("ds_read_b32 %0, %0\n\tds_read_b32 %1, %1\n\tds_read_b32 %2, %2\n\tds_read_b32 %3, %3\n\t"
                         "ds_read_b32 %4, %4\n\tds_read_b32 %5, %5\n\tds_read_b32 %6, %6\n\tds_read_b32 %7, %7\n\ts_waitcnt lgkmcnt(0)"
                         : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3), "+v"(u4), "+v"(u5), "+v"(u6), "+v"(u7) : : "memory");
        }
        x0 = (float)(u0 + u1 + u2 + u3); x1 = (float)(u4 + u5 + u6 + u7);
    } else if (KIND == 7) { // the sequence the table replaces: sqrt from rsq (5), reciprocal from rcp (3); x -> 1/sqrt(x) stays near 1
#define SEQ_OLD(x) { const float y = __builtin_amdgcn_rsqf(x); const float g = x * y, h = 0.5f * y; const float d = __builtin_fmaf(-g, g, x); \
                     const float r = __builtin_fmaf(d, h, g); const float q = __builtin_amdgcn_rcpf(r); const float e = __builtin_fmaf(-r, q, 1.0f); \
                     x = __builtin_fmaf(e, q, q); }
        for (int i = 0; i < ITERS; i++) {
            SEQ_OLD(x0) SEQ_OLD(x1) SEQ_OLD(x2) SEQ_OLD(x3) SEQ_OLD(x4) SEQ_OLD(x5) SEQ_OLD(x6) SEQ_OLD(x7)
            asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7));
        }
    } else if (KIND == 8) { // the table form: subtract, mask, shift, ds_read_b32 (and a multiply that keeps the chain going)
        if (threadIdx.x < 16) s_tab[threadIdx.x] = 0x3f800000u + ((threadIdx.x & 1u) ? 1u : 0u) - ((threadIdx.x & 2u) ? 1u : 0u);
        __syncthreads();
        x0 = x1 = x2 = x3 = x4 = x5 = x6 = x7 = 1.0f + a * 1.0e-6f;
#define SEQ_NEW(x) { const uint32_t slot = __float_as_uint(x) - 0x3f7ffff4u; x = x * __uint_as_float(s_tab[slot & 15u]); }
        for (int i = 0; i < ITERS; i++) {
            SEQ_NEW(x0) SEQ_NEW(x1) SEQ_NEW(x2) SEQ_NEW(x3) SEQ_NEW(x4) SEQ_NEW(x5) SEQ_NEW(x6) SEQ_NEW(x7)
            asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7));
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;
}

template <int KIND> void run(const char* name, float* d, double per_iter, const char* unit)
{
    for (int wps = 1; wps <= 8; wps *= 2) {
        // 256 CUs x 4 SIMDs x wps waves; blocks of 256 threads = 4 waves = one per SIMD
        const int blocks = 256 * wps;
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        hipLaunchKernelGGL(k<KIND>, dim3(blocks), dim3(256), 0, 0, d, 1.0f);
        hipDeviceSynchronize();
        hipEventRecord(e0);
        for (int r = 0; r < 5; r++) hipLaunchKernelGGL(k<KIND>, dim3(blocks), dim3(256), 0, 0, d, 1.0f);
        hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1); ms /= 5;
        const double per_simd = (double)ITERS * per_iter * wps; // wave-instructions (or sequences) issued on each SIMD
        const double cycles = ms * 1e-3 * 2.4e9;
        printf("%-44s waves/SIMD %d: %.3f ms, %.2f cycles per %s (at 2.4 GHz)\n", name, wps, ms, cycles / per_simd, unit);
        hipEventDestroy(e0); hipEventDestroy(e1);
    }
}

int main()
{
    float* d;
    if (hipMalloc(&d, 256 * 8 * 256 * sizeof(float)) != hipSuccess) { printf("no device memory\n"); return 1; }
    // run-in: an idle MI355X needs tens of milliseconds of work to reach its running clocks
    for (int r = 0; r < 500; r++) hipLaunchKernelGGL(k<0>, dim3(256 * 8), dim3(256), 0, 0, d, 1.0f);
    hipDeviceSynchronize();
    run<0>("v_mul_f32", d, 8, "wave-instruction");
    run<1>("v_rcp_f32", d, 8, "wave-instruction");
    run<2>("v_rsq_f32", d, 8, "wave-instruction");
    run<3>("v_sqrt_f32", d, 8, "wave-instruction");
    run<4>("v_mul_f64", d, 8, "wave-instruction");
    run<5>("v_cvt_f64_f32/v_cvt_f32_f64", d, 8, "wave-instruction");
    run<6>("ds_read_b32 (16 consecutive dwords)", d, 8, "wave-instruction");
    run<7>("rsq+rcp sequence (8 instr., 2 transcendental)", d, 8, "sequence");
    run<8>("table sequence (sub, and, lshl, ds_read, mul)", d, 8, "sequence");
    if (hipDeviceSynchronize() != hipSuccess) { printf("HIP error\n"); return 1; }
    hipFree(d);
    return 0;
}
