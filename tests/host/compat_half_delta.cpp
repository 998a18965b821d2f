// RayTracingManager::SetHalfDeltaFrames of include/rtx_compat.hpp, with the printer thread on a pipe.  Needs a GPU (the facade owns a
// context); tests/test_gpu_compat_half_delta.py builds it, runs one scenario per call and decodes what the printer wrote.
//
//   compat_half_delta <dir> on | whole | unprepared
//
// Three frames of the facade's default scene in RGB_PIXEL under a turning camera and a physics step each, in lock step with the
// printer.  Writes <dir>/stream.bin (every byte the printer wrote), <dir>/params.bin (the rtx_params of the last frame) and
// <dir>/last.bin (rtx_update_half's stream of the last frame, taken afterwards without a physics step).
//   on:          PrintMachine::Start(W, H, true), SetHalfDeltaFrames(true)
//   whole:       PrintMachine::Start(W, H, true), SetHalfBlocks(true) with SetDeltaFrames(true): whole frames, as before
//   unprepared:  PrintMachine::Start(W, H), then SetHalfDeltaFrames(true), which must throw; no frames
#include "rtx_compat.hpp"

#include <cstdio>
#include <fstream>

static const size_t W = 48, H = 20;

static RayTracingCPUToGPUData params_of(Camera3D& camera, float yaw_step, int i)
{
    camera.SetRot(0.0f, 3.14159274101257324f + yaw_step * (float)i, 0.0f);
    camera.Update();
    RayTracingCPUToGPUData params;
    params.inverseVMatrix = camera.GetInverseVMatrix();
    params.camPos = camera.GetPos();
    params.x = PrintMachine::GetWidth();
    params.y = PrintMachine::GetHeight();
    params.element1 = camera.GetPMatrix().row1.x;
    params.element2 = camera.GetPMatrix().row2.y;
    params.camFarDist = camera.GetFarPlaneDistance();
    return params;
}

static void save(const std::string& path, const std::string& bytes)
{
    std::ofstream f(path, std::ios::binary);
    f.write(bytes.data(), (std::streamsize)bytes.size());
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::string dir = argv[1], scenario = argv[2];
    const bool unprepared = scenario == "unprepared", whole = scenario == "whole";
    int fds[2];
    if (pipe(fds) != 0) return 2;
    std::string stream;
    std::thread reader([&] {
        char buf[4096];
        for (;;) {
            const ssize_t n = read(fds[0], buf, sizeof buf);
            if (n <= 0) break;
            stream.append(buf, (size_t)n);
        }
    });
    int rc = 0;
    try {
        PrintMachine::Start(W, H, !unprepared);
        rtx_ctx* ctx = rtx_compat::Device::get(W, H);
        RayTracingManager manager;
        Camera3D camera;
        Scene3D scene;
        camera.Init();
        scene.Init();
        manager.SetRenderingMode(RGB_PIXEL);
        if (unprepared) {
            bool threw = false;
            try {
                manager.SetHalfDeltaFrames(true);
            } catch (const std::runtime_error&) {
                threw = true;
            }
            if (!threw) throw std::runtime_error("SetHalfDeltaFrames(true) without PrintMachine::Start(x, y, true) did not throw");
        } else if (whole) {
            manager.SetHalfBlocks(true);
            manager.SetDeltaFrames(true); // (ignored while half blocks are on)
        } else {
            manager.SetHalfDeltaFrames(true);
        }
        PrintMachine::StartPrinter(fds[1], false);
        RayTracingCPUToGPUData params = params_of(camera, 0.03f, 0);
        for (int i = 0; i < 3 && !unprepared; i++) {
            params = params_of(camera, 0.03f, i);
            manager.Update(params, scene.GetObjects(), 0.05);
            PrintMachine::WaitPrinted(); // lock step
        }
        PrintMachine::StopPrinter();
        int64_t half = 0, all = 0, keys = 0, plain = 0;
        rtx_compat::check(ctx, rtx_get_option(ctx, RTX_STAT_HALF_FRAMES, &half), "rtx_get_option");
        rtx_compat::check(ctx, rtx_get_option(ctx, RTX_STAT_HALF_DELTA_FRAMES, &all), "rtx_get_option");
        rtx_compat::check(ctx, rtx_get_option(ctx, RTX_STAT_HALF_DELTA_KEYFRAMES, &keys), "rtx_get_option");
        rtx_compat::check(ctx, rtx_get_option(ctx, RTX_STAT_DELTA_FRAMES, &plain), "rtx_get_option");
        std::printf("half %lld half-delta %lld keys %lld delta %lld\n", (long long)half, (long long)all, (long long)keys, (long long)plain);
        const rtx_params p = rtx_compat::to_rtx_params(params);
        save(dir + "/params.bin", std::string(reinterpret_cast<const char*>(&p), sizeof p));
        if (!unprepared) {
            std::vector<char> own(PrintMachine::GetMaxSize());
            size_t n = 0;
            rtx_compat::check(ctx, rtx_update_half(ctx, &p, RTX_RGB_PIXEL, 0.0, 0, own.data(), own.size(), &n), "rtx_update_half");
            save(dir + "/last.bin", std::string(own.data(), n));
        }
    } catch (const std::exception& e) {
        std::printf("FAIL: %s\n", e.what());
        rc = 1;
    }
    close(fds[1]);
    reader.join();
    close(fds[0]);
    save(dir + "/stream.bin", stream);
    try {
        PrintMachine::CleanUp();
    } catch (const std::exception& e) {
        std::printf("FAIL: %s\n", e.what());
        rc = 1;
    }
    if (rc == 0) std::printf("facade half-block delta ok\n");
    return rc;
}
