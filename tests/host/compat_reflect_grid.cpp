// Scene3D::SetReflectGrid of include/rtx_compat.hpp.  Needs a GPU (the facade owns a context); tests/test_gpu_reflect_grid.py builds
// and runs it.
//
//   compat_reflect_grid
//
// The facade's default scene with two of its spheres and its plane made mirrors, depth 2, one RGB_ASCII frame through rtx_update
// (a step of no time moves nothing) in four states: the option never set; SetReflectGrid(true); the option set through the ABI
// (after SetReflectGrid(false)); SetReflectGrid(false) again.  All four streams must be the same bytes -- the option changes no
// frame -- and RTX_STAT_REFLECT_GRID_FRAMES must count the second and the third alone.
#include "rtx_compat.hpp"

#include <cstdio>
#include <string>

static const size_t W = 48, H = 20;

int main()
{
    int rc = 0;
    try {
        PrintMachine::Start(W, H);
        rtx_ctx* ctx = rtx_compat::Device::get(W, H);
        RayTracingManager manager;
        Camera3D camera;
        Scene3D scene;
        camera.Init();
        scene.Init();
        manager.SetRenderingMode(RGB_ASCII);
        scene.SetReflectivity(0, 0.5f);
        scene.SetReflectivity(2, 0.7f);
        scene.SetPlaneReflectivity(0.4f);
        scene.SetReflectDepth(2);
        camera.SetRot(0.0f, 3.14159274101257324f, 0.0f);
        camera.Update();
        RayTracingCPUToGPUData params;
        params.inverseVMatrix = camera.GetInverseVMatrix();
        params.camPos = camera.GetPos();
        params.x = PrintMachine::GetWidth();
        params.y = PrintMachine::GetHeight();
        params.element1 = camera.GetPMatrix().row1.x;
        params.element2 = camera.GetPMatrix().row2.y;
        params.camFarDist = camera.GetFarPlaneDistance();
        const rtx_params p = rtx_compat::to_rtx_params(params);
        std::vector<char> own(PrintMachine::GetMaxSize());
        const auto frame = [&](int64_t* frames, int64_t* option) {
            size_t n = 0;
            rtx_compat::check(ctx, rtx_update(ctx, &p, RTX_RGB_ASCII, 0.0, 1, own.data(), &n), "rtx_update");
            rtx_compat::check(ctx, rtx_get_option(ctx, RTX_STAT_REFLECT_GRID_FRAMES, frames), "rtx_get_option");
            rtx_compat::check(ctx, rtx_get_option(ctx, RTX_OPT_REFLECT_GRID, option), "rtx_get_option");
            return std::string(own.data(), n);
        };
        int64_t f[4] = {0, 0, 0, 0}, o[4] = {0, 0, 0, 0};
        const std::string off = frame(&f[0], &o[0]);
        scene.SetReflectGrid(true);
        const std::string facade = frame(&f[1], &o[1]);
        scene.SetReflectGrid(false);
        rtx_compat::check(ctx, rtx_set_option(ctx, RTX_OPT_REFLECT_GRID, 1), "rtx_set_option");
        const std::string abi = frame(&f[2], &o[2]);
        scene.SetReflectGrid(false);
        const std::string again = frame(&f[3], &o[3]);
        std::printf("frames off %lld facade %lld abi %lld off again %lld\n", (long long)f[0], (long long)f[1], (long long)f[2], (long long)f[3]);
        std::printf("option off %lld facade %lld abi %lld off again %lld, %zu bytes\n", (long long)o[0], (long long)o[1], (long long)o[2], (long long)o[3], off.size());
        if (o[0] != 0 || o[1] != 1 || o[2] != 1 || o[3] != 0) throw std::runtime_error("the option does not read back what was set");
        if (off.size() < 500) throw std::runtime_error("the frame is next to empty");
        if (facade != abi) throw std::runtime_error("SetReflectGrid(true) and the option set through the ABI give different frames");
        if (facade != off || again != off) throw std::runtime_error("the option changed the frame");
    } catch (const std::exception& e) {
        std::printf("FAIL: %s\n", e.what());
        rc = 1;
    }
    try {
        PrintMachine::CleanUp();
    } catch (const std::exception& e) {
        std::printf("FAIL: %s\n", e.what());
        rc = 1;
    }
    if (rc == 0) std::printf("facade reflect grid ok\n");
    return rc;
}
