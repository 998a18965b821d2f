// far_check.hip -- TEST INFRASTRUCTURE (built by __graft_entry__.build(), loaded only by tests).
// The far cut of rtx_far.hpp on the GPU: for one (num, far) per launch, all 2^32 fp32 bit patterns of dn go through
//  * the new direction test (dn > far_dir_cut(num, far), the cut computed on the device and read from LDS as the trace kernels
//    read it from their plane table) followed by div_cr, and
//  * the parent's expressions (dn > 0 || |dn| < FLT_EPSILON, then div_cr),
// and the launch counts the dn on which the two disagree in what the pixel shows of the plane: whether it is visible
// (hit, t1 > 0, t1 <= far) and, where it is, the bits of t1.  Every lane the new test alone drops is also checked against the
// compiler's IEEE division (num / dn > far) and counted.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_device.hpp"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_far.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__global__ void check_far(float num, float far, unsigned long long* mismatches, uint32_t* first_bad, unsigned long long* dropped_out, float* cut_out)
{
    __shared__ float s_cut;
    if (threadIdx.x == 0u) {
        s_cut = rtx::far_dir_cut(num, far);
        if (blockIdx.x == 0u) *cut_out = s_cut;
    }
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0, dropped = 0;
    // (every lane walks the same number of steps: div_cr votes across the wave)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const float dn = __uint_as_float((uint32_t)i);
        // the parent
        const bool out_old = dn > 0.0f || fabsf(dn - 0.0f) < 1.1920928955078125e-7f;
        // the new test, as rtx_trace_body.inc writes it
        const bool out_new = dn > s_cut;
        const float t1 = rtx::div_cr(num, dn);
        const bool vis_old = !out_old && !(t1 <= 0.0f) && t1 <= far;
        const bool vis_new = !out_new && !(t1 <= 0.0f) && t1 <= far;
        bool wrong = vis_old != vis_new || (out_old && !out_new);
        if (out_new && !out_old) {
            dropped++;
            wrong = wrong || !(rtx::div_generic(num, dn) > far);
        }
        if (wrong) {
            bad++;
            atomicMin(first_bad, (uint32_t)i);
        }
    }
    if (bad) {
        atomicAdd(mismatches, bad);
    }
    if (dropped) {
        atomicAdd(dropped_out, dropped);
    }
}

} // namespace

// Returns the number of dn on which the new direction test and the parent's differ in the plane's visible result for this
// (num, far), or on which a lane dropped by the far cut alone has num / dn <= far (0 = none on all 2^32), or -1 on a HIP error.
// *first_bad_bits: the lowest such bit pattern; *dropped: the lanes the far cut alone drops; *cut_bits: the cut the device computed.
extern "C" __attribute__((visibility("default"))) long long rtx_check_far_cut_exhaustive(float num, float far, unsigned* first_bad_bits,
                                                                                          unsigned long long* dropped, unsigned* cut_bits)
{
    unsigned long long* d_cnt = nullptr; // [0] mismatches, [1] dropped
    uint32_t* d_word = nullptr;          // [0] first bad, [1] the cut
    if (hipMalloc(&d_cnt, 16) != hipSuccess || hipMalloc(&d_word, 8) != hipSuccess) return -1;
    unsigned long long zero[2] = {0, 0};
    uint32_t words[2] = {0xffffffffu, 0u};
    hipMemcpy(d_cnt, zero, 16, hipMemcpyHostToDevice);
    hipMemcpy(d_word, words, 8, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(check_far, dim3(4096), dim3(256), 0, 0, num, far, d_cnt, d_word, d_cnt + 1, reinterpret_cast<float*>(d_word + 1));
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    unsigned long long out[2] = {0, 0};
    hipMemcpy(out, d_cnt, 16, hipMemcpyDeviceToHost);
    hipMemcpy(words, d_word, 8, hipMemcpyDeviceToHost);
    hipFree(d_cnt);
    hipFree(d_word);
    *first_bad_bits = words[0];
    *dropped = out[1];
    *cut_bits = words[1];
    return (long long)out[0];
}

// The same header evaluated by the host side of this file: the CPU's cut for the pair.
extern "C" __attribute__((visibility("default"))) float rtx_far_cut_host(float num, float far) { return rtx::far_dir_cut(num, far); }
