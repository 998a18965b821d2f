// half_check.hip -- TEST INFRASTRUCTURE (built by __graft_entry__.build(), loaded only by tests).
// Two exhaustive verifications on the GPU, each one launch over all 2^32 fp32 bit patterns that counts mismatches:
//  * half_recip() of rtx_device.hpp -- the table of rtx_unit.hpp's half_recip_bits inside the window, the generic expansion
//    outside -- returns the bits of 1.0f / (2.0f * a) (rcp_generic, the compiler's IEEE division) for EVERY a, and beside it the
//    bits of 1.0f / sqrtf(a).  The LDS tables are filled the way the trace kernels fill theirs (half_table_fill, unit_table_fill).
//  * u8_clamped(x) -- a colour channel's byte without the float clamp -- equals u8_sat(minf(255.0f, x)), the expression it replaced.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_device.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ bool same_bits_or_both_nan(float a, float b)
{
    return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
}

// POISON: one significand bit of every entry of the half-reciprocal table is flipped after the fill, so that exactly the inputs
// which half_recip answers from that table come out wrong -- the count of mismatches is then the count of table answers, taken
// from the path the helper took and not from the slot function.
template <bool POISON>
__global__ void check_half(unsigned long long* mismatches, uint32_t* first_bad, unsigned long long* from_table)
{
    __shared__ uint32_t s_half[rtx::kUnitEntries], s_unit[rtx::kUnitEntries];
    rtx::half_table_fill(s_half, threadIdx.x);
    rtx::unit_table_fill(s_unit, threadIdx.x);
    __syncthreads();
    if (POISON && threadIdx.x < rtx::kUnitEntries) s_half[threadIdx.x] ^= 0x00400000u;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0, tabled = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const float x = __uint_as_float((uint32_t)i);
        float unit;
        const float got = rtx::half_recip(x, s_half, s_unit, unit);
        const float want = rtx::rcp_generic(2.0f * x);
        if (!same_bits_or_both_nan(got, want) || !same_bits_or_both_nan(unit, 1.0f / sqrtf(x))) {
            bad++;
            atomicMin(first_bad, (uint32_t)i);
        }
        tabled += rtx::unit_slot((uint32_t)i) < rtx::kUnitEntries;
    }
    if (bad) {
        atomicAdd(mismatches, bad);
    }
    if (tabled) {
        atomicAdd(from_table, tabled);
    }
}

__global__ void check_byte(unsigned long long* mismatches, uint32_t* first_bad, unsigned long long* saturated)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0, sat = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const float x = __uint_as_float((uint32_t)i);
        const uint32_t got = rtx::u8_clamped(x);
        const uint32_t want = rtx::u8_sat(rtx::minf(255.0f, x));
        if (got != want) {
            bad++;
            atomicMin(first_bad, (uint32_t)i);
        }
        sat += got == 255u;
    }
    if (bad) {
        atomicAdd(mismatches, bad);
    }
    if (sat) {
        atomicAdd(saturated, sat);
    }
}

template <class K>
long long run(K kernel, unsigned* first_bad_bits, unsigned long long* counted)
{
    unsigned long long* d_cnt = nullptr; // [0] mismatches, [1] the kernel's second count
    uint32_t* d_first = nullptr;
    if (hipMalloc(&d_cnt, 16) != hipSuccess || hipMalloc(&d_first, 4) != hipSuccess) return -1;
    unsigned long long zero[2] = {0, 0};
    uint32_t maxu = 0xffffffffu;
    hipMemcpy(d_cnt, zero, 16, hipMemcpyHostToDevice);
    hipMemcpy(d_first, &maxu, 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(kernel, dim3(4096), dim3(256), 0, 0, d_cnt, d_first, d_cnt + 1);
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    unsigned long long out[2] = {0, 0};
    hipMemcpy(out, d_cnt, 16, hipMemcpyDeviceToHost);
    hipMemcpy(first_bad_bits, d_first, 4, hipMemcpyDeviceToHost);
    hipFree(d_cnt);
    hipFree(d_first);
    *counted = out[1];
    return (long long)out[0];
}

} // namespace

// Returns the number of inputs a on which half_recip(a) differs from 1.0f / (2.0f * a), or the rescale factor it hands out with
// it from 1.0f / sqrtf(a) (0 = both bit-identical on all 2^32), or -1 on a HIP error; *first_bad_bits: the lowest such bit pattern; *table_inputs: how many
// inputs fell inside the table's window.
extern "C" __attribute__((visibility("default"))) long long rtx_check_half_recip_exhaustive(unsigned* first_bad_bits, unsigned long long* table_inputs)
{
    return run(check_half<false>, first_bad_bits, table_inputs);
}

// The same walk with the half-reciprocal table poisoned (check_half<true>): returns the number of inputs whose divTwoA came out
// wrong, which is the number of inputs half_recip answered from its table (16 when it uses the table for exactly its window,
// 0 if it never did), or -1 on a HIP error; *first_bad_bits: the lowest of them.
extern "C" __attribute__((visibility("default"))) long long rtx_check_half_recip_poisoned(unsigned* first_bad_bits, unsigned long long* table_inputs)
{
    return run(check_half<true>, first_bad_bits, table_inputs);
}

// Returns the number of inputs x on which u8_clamped(x) differs from u8_sat(minf(255.0f, x)), or -1 on a HIP error;
// *first_bad_bits: the lowest such bit pattern; *saturated: how many inputs gave the byte 255.
extern "C" __attribute__((visibility("default"))) long long rtx_check_channel_byte_exhaustive(unsigned* first_bad_bits, unsigned long long* saturated)
{
    return run(check_byte, first_bad_bits, saturated);
}
