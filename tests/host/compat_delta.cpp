// RayTracingManager::SetDeltaFrames and PrintMachine's delta hand-off of include/rtx_compat.hpp, with the printer thread on a pipe.
// Needs a GPU (the facade owns a context); tests/test_gpu_compat_delta.py builds it, runs one scenario per call and decodes what
// the printer wrote.
//
//   compat_delta <dir> lockstep | appended | status | off
//
// Writes <dir>/stream.bin (every byte the printer wrote) and, in the delta scenarios, <dir>/frame.bin: the records of the last frame
// as rtx_render leaves them (20 W H bytes); in `off` <dir>/expected.bin: the stream the printer writes without delta frames, put
// together here from rtx_update's own bytes.
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
        PrintMachine::Start(W, H);
        rtx_ctx* ctx = rtx_compat::Device::get(W, H);
        RayTracingManager manager;
        Camera3D camera;
        Scene3D scene;
        camera.Init();
        scene.Init();
        manager.SetRenderingMode(RGB_ASCII);
        const bool off = scenario == "off", appended = scenario == "appended";
        const int frames = 4;
        if (!off) manager.SetDeltaFrames(true);
        std::string expected;
        std::vector<char> own(PrintMachine::GetMaxSize());
        if (!appended) PrintMachine::StartPrinter(fds[1], scenario == "status");
        RayTracingCPUToGPUData params;
        for (int i = 0; i < frames; i++) {
            params = params_of(camera, 0.03f, i);
            const double dt = off ? 0.0 : 0.05; // (off: a step of no time moves nothing, so rtx_update gives these bytes twice)
            if (off) {
                const rtx_params p = rtx_compat::to_rtx_params(params);
                size_t n = 0;
                rtx_compat::check(ctx, rtx_update(ctx, &p, RTX_RGB_ASCII, dt, 1, own.data(), &n), "rtx_update");
                expected += "\x1b[H" + std::string(own.data(), n) + "\x1b[m";
            }
            manager.Update(params, scene.GetObjects(), dt);
            if (!appended) PrintMachine::WaitPrinted(); // lock step
        }
        if (appended) {
            // a key frame and three deltas sit in the back buffer, unprinted: the printer takes them as one
            PrintMachine::StartPrinter(fds[1], false);
            PrintMachine::WaitPrinted();
        }
        PrintMachine::StopPrinter();
        if (off) {
            save(dir + "/expected.bin", expected);
        } else {
            const rtx_params p = rtx_compat::to_rtx_params(params);
            std::vector<char> frame(20 * W * H);
            rtx_compat::check(ctx, rtx_render(ctx, &p, RTX_RGB_ASCII), "rtx_render");
            rtx_compat::check(ctx, rtx_read_frame(ctx, frame.data(), frame.size()), "rtx_read_frame");
            save(dir + "/frame.bin", std::string(frame.data(), frame.size()));
            int64_t all = 0, keys = 0;
            rtx_compat::check(ctx, rtx_get_option(ctx, RTX_STAT_DELTA_FRAMES, &all), "rtx_get_option");
            rtx_compat::check(ctx, rtx_get_option(ctx, RTX_STAT_DELTA_KEYFRAMES, &keys), "rtx_get_option");
            std::printf("frames %lld keys %lld\n", (long long)all, (long long)keys);
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
    if (rc == 0) std::printf("facade delta ok\n");
    return rc;
}
