// RayTracingManager::SetHalfBlocks of include/rtx_compat.hpp, with the printer thread on a pipe.  Needs a GPU (the facade owns a
// context); tests/test_gpu_compat_half.py builds it, runs one scenario per call and decodes what the printer wrote.
//
//   compat_half <dir> on | off | unprepared
//
// One frame of the facade's default scene in RGB_PIXEL, in lock step with the printer.  Writes <dir>/stream.bin (every byte the
// printer wrote), <dir>/params.bin (the rtx_params of the frame) and <dir>/expected.bin (the stream put together here from the
// library's own bytes: rtx_update_half's with SetHalfBlocks(true), rtx_update's without the call).
//   on:          PrintMachine::Start(W, H, true), SetHalfBlocks(true)
//   off:         PrintMachine::Start(W, H), the call is never made
//   unprepared:  PrintMachine::Start(W, H), then SetHalfBlocks(true), which must throw
#include "rtx_compat.hpp"

#include <cstdio>
#include <fstream>

static const size_t W = 48, H = 20;

static void save(const std::string& path, const std::string& bytes)
{
    std::ofstream f(path, std::ios::binary);
    f.write(bytes.data(), (std::streamsize)bytes.size());
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::string dir = argv[1], scenario = argv[2];
    const bool on = scenario == "on";
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
        PrintMachine::Start(W, H, on);
        rtx_ctx* ctx = rtx_compat::Device::get(W, H);
        RayTracingManager manager;
        Camera3D camera;
        Scene3D scene;
        camera.Init();
        scene.Init();
        manager.SetRenderingMode(RGB_PIXEL);
        manager.SetDeltaFrames(on); // (ignored while half blocks are on)
        if (scenario == "unprepared") {
            bool threw = false;
            try {
                manager.SetHalfBlocks(true);
            } catch (const std::runtime_error&) {
                threw = true;
            }
            if (!threw) throw std::runtime_error("SetHalfBlocks(true) without PrintMachine::Start(x, y, true) did not throw");
        }
        if (on) manager.SetHalfBlocks(true);
        int64_t frames = 0;
        PrintMachine::StartPrinter(fds[1], false);
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
        size_t n = 0;
        // (a step of no time moves nothing)
        if (on) {
            rtx_compat::check(ctx, rtx_update_half(ctx, &p, RTX_RGB_PIXEL, 0.0, 1, own.data(), own.size(), &n), "rtx_update_half");
        } else {
            rtx_compat::check(ctx, rtx_update(ctx, &p, RTX_RGB_PIXEL, 0.0, 1, own.data(), &n), "rtx_update");
        }
        manager.Update(params, scene.GetObjects(), 0.0);
        PrintMachine::WaitPrinted();
        PrintMachine::StopPrinter();
        rtx_compat::check(ctx, rtx_get_option(ctx, RTX_STAT_HALF_FRAMES, &frames), "rtx_get_option");
        save(dir + "/expected.bin", "\x1b[H" + std::string(own.data(), n) + "\x1b[m");
        save(dir + "/params.bin", std::string(reinterpret_cast<const char*>(&p), sizeof p));
        std::printf("frames %lld max %zu bound %zu capacity %zu\n", (long long)frames, PrintMachine::GetMaxSize(), rtx_half_bound(RTX_RGB_PIXEL, W, H),
                    rtx_frame_capacity(ctx));
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
    if (rc == 0) std::printf("facade half blocks ok\n");
    return rc;
}
