/* Prefix header of the reference's host build: g++ reads it (-include) before every one of the reference's
 * sources, which are compiled from where they lie, unedited.
 *
 *  - pch.h first, then RayTracingManager.h before anything can include RayTracing.h: g++ refuses RayTracing.h:5's
 *    forward declaration of an unscoped enum unless the enum is already defined.
 *  - `private` and `protected` read as `public` while the reference's class definitions are read, in every
 *    translation unit alike, so that the driver reaches m_hostResultArray, Sphere::mover and speed and the
 *    scene's arrays.  Access does not change layout or code.
 *  - CUDA_KERNEL(grid, block), which pch.h:64 expands to the triple-chevron launch, becomes `* Launch{grid, block}`:
 *        kernel CUDA_KERNEL(g, b)(args...)   ==>   kernel * ref_host::Launch{g, b}(args...)
 *    Launch::operator() binds the arguments; operator*(kernel, bound) runs the kernel once per thread of the
 *    grid, in order, with blockIdx / threadIdx / blockDim set.
 *  - REF_HOST_PIN_POW (RayTracing.cu's translation unit of ref_driver_pinpow only): RayTracing.cu:73's `pow`
 *    is five squarings in double, rounded once to float, instead of the C library's powf.
 */
#pragma once
#include "pch.h"

#define private public
#define protected public
#include "RayTracingManager.h"
#include "RayTracing.h"
#include "Scene3D.h"
#include "Camera3D.h"
#include "PrintMachine.h"
#undef private
#undef protected

#include <tuple>
#include <utility>

namespace ref_host {

template <class... A>
struct Bound {
    dim3 grid, block;
    std::tuple<A...> args;
};

struct Launch {
    dim3 grid, block;
    template <class... A>
    Bound<std::decay_t<A>...> operator()(A&&... a) const
    {
        return Bound<std::decay_t<A>...>{grid, block, std::tuple<std::decay_t<A>...>(std::forward<A>(a)...)};
    }
};

template <class... P, class... A>
void operator*(void (*kernel)(P...), const Bound<A...>& b)
{
    blockDim = b.block;
    gridDim = b.grid;
    for (unsigned bz = 0; bz < b.grid.z; bz++)
    for (unsigned by = 0; by < b.grid.y; by++)
    for (unsigned bx = 0; bx < b.grid.x; bx++)
    for (unsigned tz = 0; tz < b.block.z; tz++)
    for (unsigned ty = 0; ty < b.block.y; ty++)
    for (unsigned tx = 0; tx < b.block.x; tx++) {
        blockIdx = {bx, by, bz};
        threadIdx = {tx, ty, tz};
        std::apply(kernel, b.args);
    }
}

}  // namespace ref_host

using ref_host::operator*;

#undef CUDA_KERNEL
#define CUDA_KERNEL(g, b) * ref_host::Launch{g, b}

#ifdef REF_HOST_PIN_POW
namespace ref_host {
inline float pin_pow32(float x, float /* 32.0f, RayTracing.cu:69 */)
{
    double d = (double)x;
    d = d * d;
    d = d * d;
    d = d * d;
    d = d * d;
    d = d * d;
    return (float)d;
}
}  // namespace ref_host
#define pow ref_host::pin_pow32
#endif
