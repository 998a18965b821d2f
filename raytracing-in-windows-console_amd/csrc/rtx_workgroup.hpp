// rtx_workgroup.hpp -- what the 256-thread workgroups of rtx_kernels.hip share with the files included into it and with the direct
// checks of their device code (tests/gpu_checks/cull_check.hip, tile_check.hip, sched_check.hip), which compile the same text:
// the LDS-only barrier, the workgroup's size, the spheres staged per step, the distance a pixel starts from, and the items a
// workgroup stages (the trace body and rtx_bin_cells.inc).
#pragma once

#include <hip/hip_runtime.h>

#include "rtx_kernels.h"

namespace rtx {

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the wave's outstanding
// global loads (s_waitcnt vmcnt(0)), which would expose the latency of every prefetch in flight; in
// these kernels threads exchange data through LDS alone (global memory is read-only input or
// write-only output), so waiting for LDS operations is sufficient.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

constexpr int kThreads = 256;
constexpr float kNoHit = 99999999.f; // RayTracing.h:21
constexpr int kChunk = 2 * kThreads; // spheres staged per barrier: two per thread

// The spheres a workgroup stages: all of them (list == nullptr), or the index list its coarse cell
// received from rtx_bin_cells (two-level culling for large scenes).
// A sphere is known to the trace kernels by its POSITION in the arrays they read: the direction-sorted copies when there are
// some (KArgs::sph_sorted_*), else the scene arrays themselves, where position = sphere index.  Only an exact tie in t needs the
// creation order (comes_first).
struct Items {
    const float4* geom;   // geometry by position
    const uint32_t* list; // positions (any order), or nullptr: all of [0, count)
    uint32_t count;       // number of items
};

__device__ __forceinline__ Items scene_items(const KArgs& a)
{
    Items it;
    it.geom = a.sph_geom;
    it.list = nullptr;
    it.count = a.ns;
    return it;
}

// Item i: its position and its geometry record.  Past the end any valid record is returned (ignored).
__device__ __forceinline__ float4 load_item(const Items& it, uint32_t i, uint32_t& k)
{
    if (it.count == 0u) {
        k = 0u;
        return make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const uint32_t ii = i < it.count ? i : it.count - 1u;
    k = it.list ? it.list[ii] : ii;
    return it.geom[k];
}

} // namespace rtx
