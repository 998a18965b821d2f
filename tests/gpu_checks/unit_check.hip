// unit_check.hip -- TEST INFRASTRUCTURE (built by __graft_entry__.build(), loaded only by tests).
// Exhaustive verification, on the GPU, that unit_rescale() of rtx_device.hpp -- the table of rtx_unit.hpp inside its window,
// the generic expansions outside -- returns the bits of 1.0f / sqrtf(x) for EVERY fp32 input: the kernel walks all 2^32 bit
// patterns and counts mismatches.  The LDS table is filled the way the trace kernels fill theirs (unit_table_fill).
#include "../../raytracing-in-windows-console_amd/csrc/rtx_device.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ bool same_bits_or_both_nan(float a, float b)
{
    return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
}

__global__ void check_all(unsigned long long* mismatches, uint32_t* first_bad, unsigned long long* from_table)
{
    __shared__ uint32_t s_unit[rtx::kUnitEntries];
    rtx::unit_table_fill(s_unit, threadIdx.x);
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0, tabled = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const float x = __uint_as_float((uint32_t)i);
        const float got = rtx::unit_rescale(x, s_unit);
        const float want = 1.0f / sqrtf(x);
        if (!same_bits_or_both_nan(got, want)) {
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

} // namespace

// Returns the number of inputs on which unit_rescale(x) differs from 1.0f / sqrtf(x) (0 = bit-identical on all 2^32), or -1 on a
// HIP error; *first_bad_bits: the lowest such bit pattern; *table_inputs: how many inputs fell inside the table's window.
extern "C" __attribute__((visibility("default"))) long long rtx_check_unit_rescale_exhaustive(unsigned* first_bad_bits, unsigned long long* table_inputs)
{
    unsigned long long* d_cnt = nullptr; // [0] mismatches, [1] inputs answered from the table
    uint32_t* d_first = nullptr;
    if (hipMalloc(&d_cnt, 16) != hipSuccess || hipMalloc(&d_first, 4) != hipSuccess) return -1;
    unsigned long long zero[2] = {0, 0};
    uint32_t maxu = 0xffffffffu;
    hipMemcpy(d_cnt, zero, 16, hipMemcpyHostToDevice);
    hipMemcpy(d_first, &maxu, 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(check_all, dim3(4096), dim3(256), 0, 0, d_cnt, d_first, d_cnt + 1);
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    unsigned long long out[2] = {0, 0};
    hipMemcpy(out, d_cnt, 16, hipMemcpyDeviceToHost);
    hipMemcpy(first_bad_bits, d_first, 4, hipMemcpyDeviceToHost);
    hipFree(d_cnt);
    hipFree(d_first);
    *table_inputs = out[1];
    return (long long)out[0];
}
