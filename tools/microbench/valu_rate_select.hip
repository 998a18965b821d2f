// valu_rate_select.hip -- microbenchmark (not product), sibling of valu_rate_trans.hip: issue cost on gfx950 of the instructions
// that the pass loop's guards and the record encoder are made of -- a lone v_cmp writing VCC, a lone v_cndmask_b32, v_min_u32,
// v_cvt_u32_f32, v_perm_b32, v_lshlrev_b32 in its SDWA byte-select form -- of an LDS read of one 8-byte entry among 16 against
// two 4-byte reads from two tables, and of the two whole sequences for divTwoA = 1 / (2 a): doubling, rcp, two correction FMAs
// and the range guard, against subtract, mask, shift, LDS read and window compare.
// Same form as valu_rate_trans.hip: every wave runs ITERS iterations of 8 independent chains; cycles per wave-instruction (or per
// sequence) and SIMD with 1, 2, 4, 8 waves per SIMD resident.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o valu_rate_select valu_rate_select.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
constexpr int ITERS = 4096;

#define OP8_2(TXT) asm volatile(TXT " %0, %0, %8\n\t" TXT " %1, %1, %8\n\t" TXT " %2, %2, %8\n\t" TXT " %3, %3, %8\n\t" \
                                TXT " %4, %4, %8\n\t" TXT " %5, %5, %8\n\t" TXT " %6, %6, %8\n\t" TXT " %7, %7, %8" \
                                : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(b))

template <int KIND> __global__ void k(float* out, float seed)
{
    __shared__ uint2 s_tab64[16];
    __shared__ uint32_t s_tab[2][16];
    const float a = seed + (float)(threadIdx.x & 7) * 0.125f, b = 1.0001f;
    float x0 = a + 1, x1 = a + 2, x2 = a + 3, x3 = a + 4, x4 = a + 5, x5 = a + 6, x6 = a + 7, x7 = a + 8;
    const uint32_t t = threadIdx.x;
    if (KIND == 0) { // v_mul_f32: the plain instruction everything is set against
        for (int i = 0; i < ITERS; i++) OP8_2("v_mul_f32");
    } else if (KIND == 1) { // a lone compare into VCC (nothing reads it: the cost of issuing it)
        for (int i = 0; i < ITERS; i++) {
            asm volatile("v_cmp_lt_f32 vcc, %0, %8\n\tv_cmp_lt_f32 vcc, %1, %8\n\tv_cmp_lt_f32 vcc, %2, %8\n\tv_cmp_lt_f32 vcc, %3, %8\n\t"
                         "v_cmp_lt_f32 vcc, %4, %8\n\tv_cmp_lt_f32 vcc, %5, %8\n\tv_cmp_lt_f32 vcc, %6, %8\n\tv_cmp_lt_f32 vcc, %7, %8"
                         : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(b) : "vcc");
        }
    } else if (KIND == 2) { // a lone select on a lane mask that sits in a scalar register pair, set once before the loop
        const unsigned long long mask = 0x5555555555555555ull;
        for (int i = 0; i < ITERS; i++) {
            asm volatile("v_cndmask_b32_e64 %0, %0, %8, %9\n\tv_cndmask_b32_e64 %1, %1, %8, %9\n\tv_cndmask_b32_e64 %2, %2, %8, %9\n\t"
                         "v_cndmask_b32_e64 %3, %3, %8, %9\n\tv_cndmask_b32_e64 %4, %4, %8, %9\n\tv_cndmask_b32_e64 %5, %5, %8, %9\n\t"
                         "v_cndmask_b32_e64 %6, %6, %8, %9\n\tv_cndmask_b32_e64 %7, %7, %8, %9"
                         : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(b), "s"(mask));
        }
    } else if (KIND == 3) {
        for (int i = 0; i < ITERS; i++) OP8_2("v_min_u32");
    } else if (KIND == 4) {
        for (int i = 0; i < ITERS; i++) {
            asm volatile("v_cvt_u32_f32 %0, %0\n\tv_cvt_u32_f32 %1, %1\n\tv_cvt_u32_f32 %2, %2\n\tv_cvt_u32_f32 %3, %3\n\t"
                         "v_cvt_u32_f32 %4, %4\n\tv_cvt_u32_f32 %5, %5\n\tv_cvt_u32_f32 %6, %6\n\tv_cvt_u32_f32 %7, %7"
                         : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7));
        }
    } else if (KIND == 5) {
        const uint32_t sel = 0x07060500u;
        for (int i = 0; i < ITERS; i++) {
            asm volatile("v_perm_b32 %0, %0, %8, %9\n\tv_perm_b32 %1, %1, %8, %9\n\tv_perm_b32 %2, %2, %8, %9\n\tv_perm_b32 %3, %3, %8, %9\n\t"
                         "v_perm_b32 %4, %4, %8, %9\n\tv_perm_b32 %5, %5, %8, %9\n\tv_perm_b32 %6, %6, %8, %9\n\tv_perm_b32 %7, %7, %8, %9"
                         : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(b), "v"(sel));
        }
    } else if (KIND == 6) { // shift of a selected byte: v_lshlrev_b32 with src1_sel
        const uint32_t sh = 1u;
#define SDWA(N) "v_lshlrev_b32_sdwa %" #N ", %8, %" #N " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0"
        for (int i = 0; i < ITERS; i++) {
            asm volatile(SDWA(0) "\n\t" SDWA(1) "\n\t" SDWA(2) "\n\t" SDWA(3) "\n\t" SDWA(4) "\n\t" SDWA(5) "\n\t" SDWA(6) "\n\t" SDWA(7)
                         : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(sh));
        }
    } else if (KIND == 7) { // ds_read_b64, per-lane address among 16 consecutive 8-byte entries; the low dword read is the next address
        const uint32_t base = (uint32_t)(size_t)(__attribute__((address_space(3))) void*)s_tab64;
        if (t < 16) s_tab64[t] = make_uint2(base + 8u * ((t * 5u + 3u) & 15u), t);
        __syncthreads();
        uint32_t u0 = base + 8u * (t & 15u), u1 = base + 8u * ((t + 1u) & 15u), u2 = base + 8u * ((t + 2u) & 15u), u3 = base + 8u * ((t + 3u) & 15u);
        uint32_t u4 = base + 8u * ((t + 4u) & 15u), u5 = base + 8u * ((t + 5u) & 15u), u6 = base + 8u * ((t + 6u) & 15u), u7 = base + 8u * ((t + 7u) & 15u);
        uint64_t w0, w1, w2, w3, w4, w5, w6, w7;
        uint32_t acc = 0u;
        for (int i = 0; i < ITERS; i++) {
            asm volatile("ds_read_b64 %0, %8\n\tds_read_b64 %1, %9\n\tds_read_b64 %2, %10\n\tds_read_b64 %3, %11\n\t"
                         "ds_read_b64 %4, %12\n\tds_read_b64 %5, %13\n\tds_read_b64 %6, %14\n\tds_read_b64 %7, %15\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(w0), "=&v"(w1), "=&v"(w2), "=&v"(w3), "=&v"(w4), "=&v"(w5), "=&v"(w6), "=&v"(w7)
                         : "v"(u0), "v"(u1), "v"(u2), "v"(u3), "v"(u4), "v"(u5), "v"(u6), "v"(u7) : "memory");
            // (the low halves are the next addresses: register halves, no instruction)
            u0 = (uint32_t)w0; u1 = (uint32_t)w1; u2 = (uint32_t)w2; u3 = (uint32_t)w3; u4 = (uint32_t)w4; u5 = (uint32_t)w5; u6 = (uint32_t)w6; u7 = (uint32_t)w7;
            acc ^= (uint32_t)(w0 >> 32) ^ (uint32_t)(w7 >> 32);
        }
        x0 = (float)(u0 + u1 + u2 + u3 + acc); x1 = (float)(u4 + u5 + u6 + u7);
    } else if (KIND == 8) { // two ds_read_b32 at the same slot of two 64-byte tables; the first table's entry is the next address
        const uint32_t base = (uint32_t)(size_t)(__attribute__((address_space(3))) void*)&s_tab[0][0];
        if (t < 16) { s_tab[0][t] = base + 4u * ((t * 5u + 3u) & 15u); s_tab[1][t] = t; }
        __syncthreads();
        uint32_t u0 = base + 4u * (t & 15u), u1 = base + 4u * ((t + 1u) & 15u), u2 = base + 4u * ((t + 2u) & 15u), u3 = base + 4u * ((t + 3u) & 15u);
        uint32_t u4 = base + 4u * ((t + 4u) & 15u), u5 = base + 4u * ((t + 5u) & 15u), u6 = base + 4u * ((t + 6u) & 15u), u7 = base + 4u * ((t + 7u) & 15u);
        uint32_t w0, w1, w2, w3, w4, w5, w6, w7, acc = 0u;
        for (int i = 0; i < ITERS; i++) {
            asm volatile("ds_read_b32 %8, %0 offset:64\n\tds_read_b32 %0, %0\n\tds_read_b32 %9, %1 offset:64\n\tds_read_b32 %1, %1\n\t"
                         "ds_read_b32 %10, %2 offset:64\n\tds_read_b32 %2, %2\n\tds_read_b32 %11, %3 offset:64\n\tds_read_b32 %3, %3\n\t"
                         "ds_read_b32 %12, %4 offset:64\n\tds_read_b32 %4, %4\n\tds_read_b32 %13, %5 offset:64\n\tds_read_b32 %5, %5\n\t"
                         "ds_read_b32 %14, %6 offset:64\n\tds_read_b32 %6, %6\n\tds_read_b32 %15, %7 offset:64\n\tds_read_b32 %7, %7\n\ts_waitcnt lgkmcnt(0)"
                         : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3), "+v"(u4), "+v"(u5), "+v"(u6), "+v"(u7), "=&v"(w0), "=&v"(w1), "=&v"(w2), "=&v"(w3),
                           "=&v"(w4), "=&v"(w5), "=&v"(w6), "=&v"(w7) : : "memory");
            acc ^= w0 ^ w7;
        }
        x0 = (float)(u0 + u1 + u2 + u3 + acc); x1 = (float)(u4 + u5 + u6 + u7);
    } else if (KIND == 9) { // today's divTwoA: 2a, rcp, two FMAs, and the range guard parked in a register; x -> 2 / (2x) keeps the chain near 1
        uint32_t parked = 0u;
#define SEQ_OLD(x) { const float d = x + x; const float r = __builtin_amdgcn_rcpf(d); const float e = __builtin_fmaf(-d, r, 1.0f); const float q = __builtin_fmaf(e, r, r); \
                     parked = (((__float_as_uint(d) & 0x7fffffffu) - 0x21800000u) > 0x3c000000u) ? 1u : parked; x = q + q; }
        for (int i = 0; i < ITERS; i++) {
            SEQ_OLD(x0) SEQ_OLD(x1) SEQ_OLD(x2) SEQ_OLD(x3) SEQ_OLD(x4) SEQ_OLD(x5) SEQ_OLD(x6) SEQ_OLD(x7)
            asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7), "+v"(parked));
        }
        x0 += (float)parked;
    } else if (KIND == 10) { // the table form: subtract, mask, shift, ds_read_b32, window compare (and a multiply that keeps the chain going)
        if (t < 16) s_tab[0][t] = 0x3f800000u + ((t & 1u) ? 1u : 0u) - ((t & 2u) ? 1u : 0u);
        __syncthreads();
        x0 = x1 = x2 = x3 = x4 = x5 = x6 = x7 = 1.0f + a * 1.0e-6f;
        uint32_t parked = 0u;
#define SEQ_NEW(x) { const uint32_t slot = __float_as_uint(x) - 0x3f7ffff4u; parked = slot > 15u ? 1u : parked; x = x * __uint_as_float(s_tab[0][slot & 15u]); }
        for (int i = 0; i < ITERS; i++) {
            SEQ_NEW(x0) SEQ_NEW(x1) SEQ_NEW(x2) SEQ_NEW(x3) SEQ_NEW(x4) SEQ_NEW(x5) SEQ_NEW(x6) SEQ_NEW(x7)
            asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7), "+v"(parked));
        }
        x0 += (float)parked;
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
        printf("%-52s waves/SIMD %d: %.3f ms, %.2f cycles per %s (at 2.4 GHz)\n", name, wps, ms, cycles / per_simd, unit);
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
    run<1>("v_cmp_lt_f32 -> vcc (lone)", d, 8, "wave-instruction");
    run<2>("v_cndmask_b32 (lone)", d, 8, "wave-instruction");
    run<3>("v_min_u32", d, 8, "wave-instruction");
    run<4>("v_cvt_u32_f32", d, 8, "wave-instruction");
    run<5>("v_perm_b32", d, 8, "wave-instruction");
    run<6>("v_lshlrev_b32 sdwa (src1_sel:BYTE_0)", d, 8, "wave-instruction");
    run<7>("ds_read_b64 (16 consecutive 8-byte entries)", d, 8, "wave-instruction");
    run<8>("2 x ds_read_b32 (same slot of two 64-byte tables)", d, 8, "pair");
    run<9>("2a -> rcp, 2 FMAs, range guard (divTwoA today)", d, 8, "sequence");
    run<10>("slot -> ds_read_b32, window compare (divTwoA table)", d, 8, "sequence");
    if (hipDeviceSynchronize() != hipSuccess) { printf("HIP error\n"); return 1; }
    hipFree(d);
    return 0;
}
