// check_args.hpp -- TEST INFRASTRUCTURE shared by the direct checks that take a camera in cull_check.hip's 21-float form
// (cull_check.hip, sched_check.hip): the launch arguments of such a camera, and the device copies of one call's arrays.
#pragma once

#include "../../raytracing-in-windows-console_amd/csrc/rtx_kernels.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace rtx_check {

// The launch arguments of camera `cam` for a W x H frame: the edge basis exactly as rtx_render.cpp (fill_edge_basis) fills it.
inline KArgs args_of(const float* cam, unsigned W, unsigned H)
{
    KArgs a{};
    for (int i = 0; i < 12; i++) {
        a.m[i] = cam[i];
    }
    a.ox = cam[16]; a.oy = cam[17]; a.oz = cam[18];
    a.e1 = cam[19]; a.e2 = cam[20]; a.far = 1000.0f;
    a.fW = (float)W; a.fH = (float)H;
    a.W = W; a.H = H;
    a.row0 = 0u; a.row_end = H;
    const rtxplan::EdgeBasis eb = rtxplan::edge_basis(cam, cam[19], cam[20], (uint64_t)W, (uint64_t)H);
    for (int k = 0; k < 3; k++) {
        a.edge_up_p[k] = eb.up_p[k];
        a.edge_up_q[k] = eb.up_q[k];
        a.edge_right_p[k] = eb.right_p[k];
        a.edge_right_q[k] = eb.right_q[k];
        a.edge_fwd[k] = eb.fwd[k];
    }
    a.edge_pp = eb.pp;
    a.edge_qrqr = eb.qrqr;
    a.edge_qcqc = eb.qcqc;
    return a;
}

// Device copies of the inputs and outputs of one call, freed when it returns.
struct Buffers {
    std::vector<void*> held;
    bool ok = true;
    void* up(const void* src, size_t bytes)
    {
        void* d = nullptr;
        ok = ok && hipMalloc(&d, bytes ? bytes : 4) == hipSuccess;
        if (ok) held.push_back(d);
        ok = ok && (src == nullptr ? hipMemset(d, 0, bytes ? bytes : 4) : hipMemcpy(d, src, bytes, hipMemcpyHostToDevice)) == hipSuccess;
        return d;
    }
    bool down(void* dst, const void* d, size_t bytes) { return ok = ok && hipMemcpy(dst, d, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
    bool ran() { return ok = ok && hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess; }
    ~Buffers()
    {
        for (void* d : held) hipFree(d);
    }
};

} // namespace rtx_check
