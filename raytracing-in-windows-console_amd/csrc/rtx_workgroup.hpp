// rtx_workgroup.hpp -- what the 256-thread workgroups of rtx_kernels.hip share with the files included into it and with the direct
// checks of their device code (tests/gpu_checks/cull_check.hip, tests/gpu_checks/tile_check.hip), which compile the same text:
// the LDS-only barrier, the workgroup's size, the spheres staged per step and the distance a pixel starts from.
#pragma once

#include <hip/hip_runtime.h>

namespace rtx {

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the wave's outstanding
// global loads (s_waitcnt vmcnt(0)), which would expose the latency of every prefetch in flight; in
// these kernels threads exchange data through LDS alone (global memory is read-only input or
// write-only output), so waiting for LDS operations is sufficient.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

constexpr int kThreads = 256;
constexpr float kNoHit = 99999999.f; // RayTracing.h:21
constexpr int kChunk = 2 * kThreads; // spheres staged per barrier: two per thread

} // namespace rtx
