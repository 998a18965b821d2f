/* Stand-in for <cuda_runtime.h>: enough of the runtime for the reference's sources to compile and run as
 * plain host C++.  "Device" memory is host memory; a kernel launch is a loop (see ../prefix.h). */
#pragma once
#include <cfloat>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#define __host__
#define __device__
#define __global__
#define __constant__

struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct ref_host_uint3 {
    unsigned int x, y, z;
};
/* the indices of the "thread" the launch loop is running */
inline thread_local ref_host_uint3 blockIdx = {0, 0, 0};
inline thread_local ref_host_uint3 threadIdx = {0, 0, 0};
inline thread_local dim3 blockDim;
inline thread_local dim3 gridDim;

enum cudaError_t { cudaSuccess = 0, cudaErrorMemoryAllocation = 2 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };

inline const char* cudaGetErrorString(cudaError_t e) { return e == cudaSuccess ? "no error" : "out of memory"; }

template <class T>
inline cudaError_t cudaMalloc(T** p, size_t n)
{
    *p = static_cast<T*>(std::malloc(n ? n : 1));
    return *p ? cudaSuccess : cudaErrorMemoryAllocation;
}
inline cudaError_t cudaMemcpy(void* dst, const void* src, size_t n, cudaMemcpyKind)
{
    std::memcpy(dst, src, n);
    return cudaSuccess;
}
inline cudaError_t cudaMemset(void* p, int v, size_t n)
{
    std::memset(p, v, n);
    return cudaSuccess;
}
inline cudaError_t cudaFree(void* p)
{
    std::free(p);
    return cudaSuccess;
}
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
