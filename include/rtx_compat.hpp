// rtx_compat.hpp -- the reference's C++ API surface for the ray-trace path, rebuilt over the C ABI.
//
// Header-only host code.  It keeps the names, signatures, argument meaning and call order of the
// reference's classes so that Engine3D-style plumbing (Engine3D.cpp:9-28, 81-107) compiles against
// it unchanged, while every device-side action goes through include/rtx.h into librtx_hip.so:
//
//   MyMath::Vector3 / Vector4 / Matrix      MyMath.h:5-321   (PODs here: no vptrs travel to the GPU)
//   DeviceObjectArray<T>, Object3D          Object3D.h:6-12, 36-65 (opaque handle here)
//   RayTracingCPUToGPUData, RenderingMode   RayTracingManager.h:9-21
//   PrintMachine                            PrintMachine.h:16-45: Start, GetMaxSize, GetWidth, GetHeight,
//                                           SetDataInBackBuffer, GetBackBuffer, GetPrintSize; the printer thread
//                                           (PrintMachine.cpp:257-306) for a POSIX terminal via StartPrinter(fd)
//   Scene3D                                 Scene3D.h:15-25
//   Camera3D                                Camera3D.h:12-48 (Init, Update, Move, AddRot, m_Keys, SetRot, SetPos, getters)
//   RayTracingManager                       RayTracingManager.h:27-37
//   RayTracing::RayTrace                    RayTracing.h:31-38
//
// Differences, all deliberate: errors throw std::runtime_error with the library's message instead of
// exit() (pch.h:45-53); Scene3D has no 5 MB arena cap (Scene3D.h:6); Sphere speed is not drawn from
// rand() (Sphere.cu:11-12) but defaults to 1 and can be set; RayTracing::RayTrace takes the params as a
// HOST pointer (they travel as kernel arguments) and ignores gridDims/blockDims (tiling is chosen
// for gfx950 inside the library).
#pragma once

#include "rtx.h"

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

namespace MyMath {

struct Vector3 {
    float x = 0.0f, y = 0.0f, z = 0.0f;
    Vector3() = default;
    Vector3(float inX, float inY, float inZ) : x(inX), y(inY), z(inZ) {}
    Vector3(int inX, int inY, int inZ) : x((float)inX), y((float)inY), z((float)inZ) {}
    Vector3 operator-(const Vector3& o) const { return Vector3(x - o.x, y - o.y, z - o.z); }
    Vector3 operator+(const Vector3& o) const { return Vector3(x + o.x, y + o.y, z + o.z); }
    Vector3 operator*(float s) const { return Vector3(x * s, y * s, z * s); }
    Vector3 operator/(float s) const { return Vector3(x / s, y / s, z / s); }
};

struct Vector4 {
    float x = 0.0f, y = 0.0f, z = 0.0f, w = 0.0f;
    Vector4() = default;
    Vector4(float inX, float inY, float inZ, float inW) : x(inX), y(inY), z(inZ), w(inW) {}
    Vector4(const Vector3& v, float inW) : x(v.x), y(v.y), z(v.z), w(inW) {}
    Vector3 xyz() const { return Vector3(x, y, z); }
};

struct Matrix {
    Vector4 row1, row2, row3, row4;
    Matrix() = default;
    Matrix(const Vector4& a, const Vector4& b, const Vector4& c, const Vector4& d) : row1(a), row2(b), row3(c), row4(d) {}
    Vector4 Mult(const Vector4& v) const
    {
        return Vector4(row1.x * v.x + row1.y * v.y + row1.z * v.z + row1.w * v.w,
                       row2.x * v.x + row2.y * v.y + row2.z * v.z + row2.w * v.w,
                       row3.x * v.x + row3.y * v.y + row3.z * v.z + row3.w * v.w,
                       row4.x * v.x + row4.y * v.y + row4.z * v.z + row4.w * v.w);
    }
};

inline float Dot(const Vector3& a, const Vector3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

} // namespace MyMath

// ---------------------------------------------------------------------------------------------

class Object3D; // opaque: objects live in the library's SoA store

template <typename T>
struct DeviceObjectArray {
    T* m_deviceArray = nullptr; // here: an opaque handle to the scene store of the shared context
    unsigned int allocatedBytes = 0;
    unsigned int count = 0;
};

struct RayTracingCPUToGPUData {
    MyMath::Matrix inverseVMatrix;
    MyMath::Vector3 camPos;
    size_t x = 0;
    size_t y = 0;
    float element1 = 0.0f;
    float element2 = 0.0f;
    float camFarDist = 0.0f;
};

enum RenderingMode { BIT_ASCII = 0, BIT_PIXEL, RGB_ASCII, RGB_PIXEL, RGB_NORMALS, SDL };

struct dim3_compat {
    unsigned x = 1, y = 1, z = 1;
    dim3_compat() = default;
    dim3_compat(unsigned a, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};

namespace rtx_compat {

inline rtx_params to_rtx_params(const RayTracingCPUToGPUData& p)
{
    rtx_params r;
    const MyMath::Vector4* rows[4] = {&p.inverseVMatrix.row1, &p.inverseVMatrix.row2, &p.inverseVMatrix.row3, &p.inverseVMatrix.row4};
    for (int i = 0; i < 4; i++) {
        r.inv_v[4 * i + 0] = rows[i]->x;
        r.inv_v[4 * i + 1] = rows[i]->y;
        r.inv_v[4 * i + 2] = rows[i]->z;
        r.inv_v[4 * i + 3] = rows[i]->w;
    }
    r.cam_pos[0] = p.camPos.x;
    r.cam_pos[1] = p.camPos.y;
    r.cam_pos[2] = p.camPos.z;
    r.element1 = p.element1;
    r.element2 = p.element2;
    r.cam_far = p.camFarDist;
    r.x = p.x;
    r.y = p.y;
    return r;
}

inline void check(rtx_ctx* ctx, int status, const char* what)
{
    if (status != RTX_OK) {
        throw std::runtime_error(std::string(what) + ": " + rtx_last_error(ctx));
    }
}

// One device context per process, like the reference's single default device -- or one device GROUP: with a
// device list (Device::set_devices({0, 1, 2, 3}) before the first use, or RTX_DEVICES=0,1,2,3 in the environment) the same
// context renders every frame row-sharded over those GPUs and assembles it on the first (rtx_group_create, rtx.h), and
// Engine3D::Render-style code -- Scene3D::CreateSphere, RayTracingManager::Update -- runs unchanged on top.
struct Device {
    static rtx_ctx*& slot()
    {
        static rtx_ctx* ctx = nullptr;
        return ctx;
    }
    static int& ordinal()
    {
        static int dev = 0;
        return dev;
    }
    static std::vector<int>& devices()
    {
        static std::vector<int> list;
        return list;
    }
    static void set_devices(const std::vector<int>& list) { devices() = list; }
    // Pixel rows per console row the context is created for: 1, or 2 for half-block frames (PrintMachine::Start(x, y, true);
    // rtx_update_half traces W x 2H pixels).  Read when the context is created.
    static size_t& rows_per_cell()
    {
        static size_t rows = 1;
        return rows;
    }
    static std::vector<int> devices_from_environment()
    {
        std::vector<int> list;
        const char* env = std::getenv("RTX_DEVICES");
        if (!env) return list;
        const char* p = env;
        while (*p) {
            char* end = nullptr;
            const long v = std::strtol(p, &end, 10);
            if (end == p) break;
            list.push_back((int)v);
            p = end;
            while (*p == ',' || *p == ' ') p++;
        }
        return list;
    }
    static rtx_ctx* get(size_t max_w, size_t max_h)
    {
        rtx_ctx*& ctx = slot();
        if (!ctx) {
            std::vector<int> list = devices().empty() ? devices_from_environment() : devices();
            const size_t rows = max_h * rows_per_cell();
            const int rc = list.empty() ? rtx_create(ordinal(), max_w, rows, &ctx)
                                        : rtx_group_create((int)list.size(), list.data(), max_w, rows, &ctx);
            if (rc != RTX_OK) {
                throw std::runtime_error(std::string(list.empty() ? "rtx_create: " : "rtx_group_create: ") + rtx_last_error(nullptr));
            }
        }
        return ctx;
    }
    static void release()
    {
        if (slot()) {
            rtx_destroy(slot());
            slot() = nullptr;
        }
    }
};

} // namespace rtx_compat

// ---------------------------------------------------------------------------------------------
// PrintMachine: the statics the hot path calls (RayTracingManager.cu:58,150,306) with the double buffer and mutex of
// PrintMachine.cpp:178-192, and -- on request -- the printer thread of PrintMachine.cpp:257-306 for a POSIX
// terminal: StartPrinter(fd) spawns it; it swaps the back buffer in under the mutex, homes the cursor with an ANSI
// escape (the reference calls SetConsoleCursorPosition(0,0)) and writes the frame to fd.  Without StartPrinter the
// class is headless (the caller reads GetBackBuffer / GetPrintSize itself).  One deliberate difference: the
// reference's thread re-prints the same buffer in a busy loop between frames; this one sleeps on a condition
// variable until SetDataInBackBuffer flags a new frame (a terminal gains nothing from identical bytes), and a frame
// that arrives while the previous one is still being written replaces it, as in the reference.  With delta frames
// (SetDeltaInBackBuffer) the cursor is homed in front of key frames only.  Start(x, y, true) prepares for half-block frames
// (RayTracingManager::SetHalfBlocks; no reference counterpart): the buffers are sized by rtx_half_bound -- 41 bytes per cell
// where a frame of records has 20 -- and the device context is created for 2 y pixel rows.
class PrintMachine {
public:
    static void Start(const size_t x, const size_t y, const bool half_blocks = false)
    {
        State& s = state();
        s.width = x;
        s.height = y;
        s.maxSize = 20 * x * y; // m_charsPerPixel, PrintMachine.h:81
        s.halfBlocks = half_blocks;
        if (half_blocks) {
            const size_t bound = rtx_half_bound(RTX_RGB_PIXEL, x, y); // (the longer family's: the mode may change while running)
            if (bound == 0) throw std::runtime_error("PrintMachine::Start: no half-block frames of this size");
            if (bound > s.maxSize) s.maxSize = bound;
        }
        rtx_compat::Device::rows_per_cell() = half_blocks ? 2 : 1;
        s.backBuffer.assign(s.maxSize, 0);
        s.printBuffer.assign(s.maxSize, 0);
        s.backBufferPrintSize = 0;
        s.shouldSwap = false;
    }
    static void CleanUp()
    {
        StopPrinter();
        rtx_compat::Device::release();
    }
    static size_t GetWidth() { return state().width; }
    static size_t GetHeight() { return state().height; }
    static size_t GetMaxSize() { return state().maxSize; }
    static bool HalfBlocks() { return state().halfBlocks; }
    static bool ChangeSize(const size_t x, const size_t y)
    {
        state().width = x;
        state().height = y;
        return true;
    }
    static void SetDataInBackBuffer(const char* data, const size_t size)
    {
        State& s = state();
        {
            std::lock_guard<std::mutex> lock(s.mutex);
            std::memcpy(s.backBuffer.data(), data, size);
            s.shouldSwap = true; // FlagForBufferSwap
            s.backBufferPrintSize = size;
            s.backIsKey = true;
            s.framesSet++;
        }
        s.wake.notify_all();
    }
    // Delta frames (RayTracingManager::SetDeltaFrames; rtx_update_delta in rtx.h).  No reference counterpart: its printer rewrites the
    // whole screen (PrintMachine.cpp:257-306).  A key frame replaces the back buffer, as SetDataInBackBuffer does.  A delta that
    // arrives while an unprinted frame still sits in the back buffer is APPENDED to it -- deltas applied in order are correct,
    // replacing one is not -- and where that would exceed GetMaxSize() nothing is taken and false is returned: the caller hands
    // in a key frame instead.
    static bool SetDeltaInBackBuffer(const char* data, const size_t size, const bool key)
    {
        State& s = state();
        {
            std::lock_guard<std::mutex> lock(s.mutex);
            const size_t at = (!key && s.shouldSwap) ? s.backBufferPrintSize : 0;
            if (at + size > s.maxSize) return false;
            std::memcpy(s.backBuffer.data() + at, data, size);
            if (at == 0) s.backIsKey = key;
            s.shouldSwap = true;
            s.backBufferPrintSize = at + size;
            s.framesSet++;
        }
        s.wake.notify_all();
        return true;
    }
    // In delta mode the printer does not rely on where a frame leaves the cursor: the status lines are addressed to row H + 1.
    static void SetDeltaMode(const bool on)
    {
        State& s = state();
        std::lock_guard<std::mutex> lock(s.mutex);
        s.deltaMode = on;
    }
    static const char* GetBackBuffer() { return state().backBuffer.data(); }
    static size_t GetPrintSize() { return state().backBufferPrintSize; }
    static void UpdateRenderingFPS(const int fps) { state().renderingFps = fps; }

    // ---- the printer thread (PrintMachine::Start spawns and detaches it, PrintMachine.cpp:150-151; here it is joined
    // by StopPrinter / CleanUp).  status_lines: print the two FPS lines after every frame as the reference does.
    static void StartPrinter(int fd, bool status_lines = true)
    {
        State& s = state();
        if (s.printer.joinable()) return;
        s.fd = fd;
        s.statusLines = status_lines;
        s.terminate = false;
        s.printer = std::thread(&PrintMachine::Print);
    }
    static void StopPrinter()
    {
        State& s = state();
        if (!s.printer.joinable()) return;
        {
            std::lock_guard<std::mutex> lock(s.mutex);
            s.terminate = true; // m_terminateThread
        }
        s.wake.notify_all();
        s.printer.join();
    }
    // Blocks until every frame handed to SetDataInBackBuffer so far has been written (a lock-step caller: tests).
    static void WaitPrinted()
    {
        State& s = state();
        std::unique_lock<std::mutex> lock(s.mutex);
        s.done.wait(lock, [&] { return s.framesPrinted == s.framesSet || !s.printer.joinable() || s.terminate; });
    }
    static unsigned long long FramesPrinted() { return state().framesPrinted; }

private:
    static void write_all(int fd, const char* p, size_t n)
    {
        while (n > 0) {
            const ssize_t w = ::write(fd, p, n);
            if (w < 0) {
                if (errno == EINTR || errno == EAGAIN) continue;
                return; // the terminal went away
            }
            p += w;
            n -= (size_t)w;
        }
    }
    static bool Print() // PrintMachine.cpp:257-306
    {
        State& s = state();
        auto second = std::chrono::steady_clock::now();
        int printed_this_second = 0, printing_fps = 0;
        for (;;) {
            size_t size = 0;
            unsigned long long upto = 0;
            bool key = true, delta_mode = false;
            {
                std::unique_lock<std::mutex> lock(s.mutex);
                s.wake.wait(lock, [&] { return s.shouldSwap || s.terminate; });
                if (s.terminate && !s.shouldSwap) break;
                s.shouldSwap = false;
                size = s.backBufferPrintSize;     // m_printSize = m_backBufferPrintSize
                s.printBuffer.swap(s.backBuffer); // m_printBuffer.swap(m_backBuffer)
                upto = s.framesSet;
                key = s.backIsKey;
                delta_mode = s.deltaMode;
            }
            if (key) write_all(s.fd, "\x1b[H", 3); // ResetConsolePointer: cursor home (a delta addresses its own cells)
            write_all(s.fd, s.printBuffer.data(), size);
            printed_this_second++;
            const auto now = std::chrono::steady_clock::now();
            if (now - second >= std::chrono::seconds(1)) {
                printing_fps = printed_this_second;
                printed_this_second = 0;
                second = now;
            }
            if (s.statusLines) {
                char line[160];
                int n = 0;
                if (delta_mode) n = std::snprintf(line, sizeof line, "\x1b[%zu;1H", s.height + 1); // (a delta leaves the cursor anywhere)
                n += std::snprintf(line + n, sizeof line - (size_t)n, "\x1b[mRendering FPS: %d    \nPrinting FPS: %d    \n", s.renderingFps, printing_fps);
                write_all(s.fd, line, (size_t)n);
            } else {
                write_all(s.fd, "\x1b[m", 3);
            }
            {
                std::lock_guard<std::mutex> lock(s.mutex);
                s.framesPrinted = upto;
            }
            s.done.notify_all();
        }
        s.done.notify_all();
        return true;
    }
    struct State {
        size_t width = 0, height = 0, maxSize = 0, backBufferPrintSize = 0;
        std::vector<char> backBuffer, printBuffer;
        std::mutex mutex; // m_backBufferMutex
        std::condition_variable wake, done;
        bool shouldSwap = false, terminate = false, statusLines = true;
        bool backIsKey = true;  // the back buffer starts with a whole frame (else with a delta: no cursor home in front of it)
        bool deltaMode = false; // SetDeltaMode
        bool halfBlocks = false; // Start(x, y, true)
        unsigned long long framesSet = 0, framesPrinted = 0;
        int fd = 1, renderingFps = 0;
        std::thread printer;
    };
    static State& state()
    {
        static State s;
        return s;
    }
};

// ---------------------------------------------------------------------------------------------
class Scene3D {
public:
    void Init()
    {
        ctx();
        check(rtx_scene_clear(ctx()), "rtx_scene_clear");
        m_planes.clear();
        // the reference's start scene, Scene3D.cpp:28-33
        CreateSphere(7.0f, MyMath::Vector3(0.0f, 10.0f, 20.0f), MyMath::Vector3(255.0f, 1.0f, 1.0f));
        CreateSphere(6.0f, MyMath::Vector3(5.0f, 10.0f, 20.0f), MyMath::Vector3(1.0f, 255.0f, 1.0f));
        CreateSphere(10.0f, MyMath::Vector3(10.0f, 10.0f, 40.0f), MyMath::Vector3(1.0f, 1.0f, 255.0f));
        CreateSphere(3.0f, MyMath::Vector3(5.0f, 10.0f, 20.0f), MyMath::Vector3(225.0f, 210.0f, 20.0f));
        CreateSphere(4.0f, MyMath::Vector3(-5.0f, 10.0f, 40.0f), MyMath::Vector3(225.0f, 10.0f, 220.0f));
        CreatePlane(MyMath::Vector3(0.0f, -3.0f, 30.0f), MyMath::Vector3(0.0f, 1.0f, 0.0f), MyMath::Vector3(100.0f, 100.0f, 100.0f), 10, 20);
    }
    void Update(const long double) {} // the GPU updates objects (Scene3D.cpp:89-92)
    void CleanUp()
    {
        check(rtx_scene_clear(ctx()), "rtx_scene_clear");
        m_planes.clear();
    }

    void CreatePlane(const MyMath::Vector3& middlePos, const MyMath::Vector3& normal, const MyMath::Vector3& color,
                     const float width, const float height)
    {
        const float p[3] = {middlePos.x, middlePos.y, middlePos.z}, n[3] = {normal.x, normal.y, normal.z}, c[3] = {color.x, color.y, color.z};
        const int idx = rtx_scene_add_plane(ctx(), p, n, c, width, height);
        if (idx < 0) check(-idx, "rtx_scene_add_plane");
        m_planes.push_back((unsigned)idx); // (creation indices only grow)
    }
    void CreateSphere(const float radius, const MyMath::Vector3& middlePos, const MyMath::Vector3& color)
    {
        const float p[3] = {middlePos.x, middlePos.y, middlePos.z}, c[3] = {color.x, color.y, color.z};
        const int idx = rtx_scene_add_sphere(ctx(), p, radius, c);
        if (idx < 0) check(-idx, "rtx_scene_add_sphere");
    }
    // Extensions, no reference counterpart (RayTracing.cu:635 plans a recursive RayTrace): one-bounce mirrors, k in [0, 1] for the
    // object of creation index `index` (rtx_scene_set_reflectivity), or for every plane this scene created -- one call over the
    // range they span, the values of the objects between them read back from the host copy (rtx_scene_get_reflectivity).
    void SetReflectivity(const unsigned index, const float k) { check(rtx_scene_set_reflectivity(ctx(), index, 1, &k), "rtx_scene_set_reflectivity"); }
    void SetPlaneReflectivity(const float k)
    {
        if (m_planes.empty()) return;
        const unsigned first = m_planes.front(), last = m_planes.back();
        std::vector<float> v(last - first + 1);
        for (unsigned i = first; i <= last; i++) check(rtx_scene_get_reflectivity(ctx(), i, &v[i - first]), "rtx_scene_get_reflectivity");
        for (const unsigned i : m_planes) v[i - first] = k;
        check(rtx_scene_set_reflectivity(ctx(), first, v.size(), v.data()), "rtx_scene_set_reflectivity");
    }
    // Extension, no reference counterpart (RayTracing.cu:635): glass.  The index of refraction of the object of creation index `index`
    // (rtx_scene_set_refraction: 0 a mirror, else in [1, 4]); it shows where the object's reflectivity is above 0.
    void SetRefraction(const unsigned index, const float ior) { check(rtx_scene_set_refraction(ctx(), index, 1, &ior), "rtx_scene_set_refraction"); }
    // Extension, no reference counterpart (RayTracing.cu:73,143-157 shade every object with the same constants): the surface finish of
    // the object of creation index `index` (rtx_scene_set_finish: the weights of its own colour under no light, of the lights'
    // diffuse terms and of their highlights, each in [0, 16], and the Blinn-Phong exponent 2^shininess_log2, at most 2^8).
    void SetFinish(const unsigned index, const float ambient, const float diffuse, const float specular, const unsigned shininess_log2)
    {
        const rtx_finish f = {ambient, diffuse, specular, shininess_log2};
        check(rtx_scene_set_finish(ctx(), index, 1, &f), "rtx_scene_set_finish");
    }
    // Extension, no reference counterpart (the reference casts no shadows): whether the object of creation index `index` counts as an
    // occluder in the shadow tests (rtx_scene_set_shadow_casting; every new object does).  It is seen, lit and shadowed either way.
    void SetCastsShadow(const unsigned index, const bool casts)
    {
        const uint8_t cast = casts ? 1u : 0u;
        check(rtx_scene_set_shadow_casting(ctx(), index, 1, &cast), "rtx_scene_set_shadow_casting");
    }
    // Extensions, no reference counterpart (RayTracing.cu:144 reads the one colour an object has): checker patterns.  The table of
    // up to RTX_MAX_PATTERNS entries (rtx_scene_set_patterns; entry i serves slot i + 1), the slot of the object of creation index
    // `index` (0: none), or of every plane this scene created (rtx_scene_set_object_pattern, a call per plane: the objects between
    // them keep theirs).
    void SetPatterns(const rtx_pattern* patterns, const size_t n) { check(rtx_scene_set_patterns(ctx(), n, patterns), "rtx_scene_set_patterns"); }
    void SetPattern(const unsigned index, const unsigned slot) { check(rtx_scene_set_object_pattern(ctx(), index, 1, slot), "rtx_scene_set_object_pattern"); }
    void SetPlanePattern(const unsigned slot)
    {
        for (const unsigned i : m_planes) check(rtx_scene_set_object_pattern(ctx(), i, 1, slot), "rtx_scene_set_object_pattern");
    }
    // Mirrors that see mirrors: levels of secondary rays, 1 .. RTX_MAX_REFLECT_DEPTH (RTX_OPT_REFLECT_DEPTH).
    // No reference counterpart (RayTracing.cu:635).
    void SetReflectDepth(const int depth) { check(rtx_set_option(ctx(), RTX_OPT_REFLECT_DEPTH, depth), "RTX_OPT_REFLECT_DEPTH"); }
    int GetReflectDepth()
    {
        int64_t v = 1;
        check(rtx_get_option(ctx(), RTX_OPT_REFLECT_DEPTH, &v), "RTX_OPT_REFLECT_DEPTH");
        return (int)v;
    }
    // Mirror rays through the ray queries' world grid instead of the tiles' bundles (RTX_OPT_REFLECT_GRID): the same frames, byte for
    // byte; off by default.  No reference counterpart (RayTracing.cu:635).
    void SetReflectGrid(const bool on) { check(rtx_set_option(ctx(), RTX_OPT_REFLECT_GRID, on ? 1 : 0), "RTX_OPT_REFLECT_GRID"); }
    // Objects edited in place, by creation index.  The reference has the seam -- Object3D::SetMiddlePos (Object3D.h:55,
    // Object3D.cu:34) -- and never calls it after upload; here a sphere takes a new centre, radius and colour (rtx_scene_set_spheres:
    // rows of cx cy cz r R G B for first .. first+n-1), a plane all its fields (rtx_scene_set_plane).  Mover, speed, reflectivity
    // and the creation order stay.
    void SetSphere(const unsigned index, const float radius, const MyMath::Vector3& middlePos, const MyMath::Vector3& color)
    {
        const float row[7] = {middlePos.x, middlePos.y, middlePos.z, radius, color.x, color.y, color.z};
        check(rtx_scene_set_spheres(ctx(), index, 1, row), "rtx_scene_set_spheres");
    }
    void SetSpheres(const unsigned first, const size_t n, const float* xyzr_rgb) { check(rtx_scene_set_spheres(ctx(), first, n, xyzr_rgb), "rtx_scene_set_spheres"); }
    void SetPlane(const unsigned index, const MyMath::Vector3& middlePos, const MyMath::Vector3& normal, const MyMath::Vector3& color,
                  const float width, const float height)
    {
        const float p[3] = {middlePos.x, middlePos.y, middlePos.z}, n[3] = {normal.x, normal.y, normal.z}, c[3] = {color.x, color.y, color.z};
        check(rtx_scene_set_plane(ctx(), index, p, n, c, width, height), "rtx_scene_set_plane");
    }
    // Objects removed, by creation index (rtx_scene_remove_objects: any order, no duplicates; all or nothing).  No reference
    // counterpart: Scene3D.h:15-25 creates objects and Scene3D::CleanUp frees all of them at once.  A survivor of old index i is
    // object i - |{r removed : r < i}| afterwards: callers renumber what they hold by that rule, as m_planes is here.
    void RemoveObjects(const size_t n, const unsigned* indices)
    {
        check(rtx_scene_remove_objects(ctx(), n, indices), "rtx_scene_remove_objects");
        std::vector<unsigned> gone(indices, indices + n), planes;
        std::sort(gone.begin(), gone.end());
        for (const unsigned i : m_planes) {
            const auto at = std::lower_bound(gone.begin(), gone.end(), i);
            if (at == gone.end() || *at != i) planes.push_back(i - (unsigned)(at - gone.begin()));
        }
        m_planes.swap(planes);
    }
    void RemoveObject(const unsigned index) { RemoveObjects(1, &index); }
    DeviceObjectArray<Object3D*> GetObjects()
    {
        DeviceObjectArray<Object3D*> a;
        a.m_deviceArray = reinterpret_cast<Object3D**>(ctx());
        a.count = rtx_scene_count(ctx());
        a.allocatedBytes = a.count * (unsigned)sizeof(void*);
        return a;
    }

private:
    static rtx_ctx* ctx() { return rtx_compat::Device::get(PrintMachine::GetWidth(), PrintMachine::GetHeight()); }
    static void check(int status, const char* what) { rtx_compat::check(ctx(), status, what); }
    std::vector<unsigned> m_planes; // creation indices of the planes CreatePlane added since the last clear
};

// ---------------------------------------------------------------------------------------------
// Camera3D: the pure host math that produces the path's input (Camera3D.cpp:8-98, 207-376), through
// rtx_camera_params so that there is one implementation of it.
class Camera3D {
public:
    struct PressedKeys { // Camera3D.h:37-46
        int W = 0, A = 0, S = 0, D = 0, Shift = 0, Space = 0;
    };
    PressedKeys m_Keys;

    void Init() { refresh(); }
    void Update() { refresh(); }
    // Camera3D::Move, Camera3D.cpp:142-163: WASD in the x-z plane along the "static" right / forward vectors of the last
    // Update (:61-71; their y components take no part), Space / Shift along y; speed 10 units per second; the summed
    // direction is normalised with the safe host normalise (MyMath.h:117-123), so diagonals are not faster.
    void Move(const long double dt)
    {
        const float deltaSpeed = static_cast<float>(dt) * 10.0f;
        const MyMath::Vector3 moveX = m_staticRight * static_cast<float>(m_Keys.D - m_Keys.A);
        const MyMath::Vector3 moveZ = m_staticForward * static_cast<float>(m_Keys.W - m_Keys.S);
        MyMath::Vector3 total = moveX + moveZ;
        const float length = std::sqrt(total.x * total.x + total.y * total.y + total.z * total.z);
        const float divider = length < 0.000001f ? 0.0f : 1.0f / length;
        total = total * divider;
        m_pos.x = m_pos.x + (total.x * deltaSpeed);
        m_pos.z = m_pos.z + (total.z * deltaSpeed);
        m_pos.y += (float)(m_Keys.Space - m_Keys.Shift) * deltaSpeed;
    }
    // Camera3D::AddRot, Camera3D.cpp:166-187: p / y / r are mouse counts; 0.002 rad per count whatever dt; pitch clamped
    // just inside +-pi/2.
    void AddRot(const long double, const short p, const short y, const short r)
    {
        const float deltaSpeed = 0.002f;
        m_rot.x -= ((float)p * deltaSpeed);
        m_rot.y += ((float)y * deltaSpeed);
        m_rot.z += ((float)r * deltaSpeed);
        if (m_rot.x > static_cast<float>(3.14159265358979323846 / 2.0)) m_rot.x = static_cast<float>((3.14159265358979323846 / 2.0) - 0.0001);
        if (m_rot.x < static_cast<float>(-3.14159265358979323846 / 2.0)) m_rot.x = static_cast<float>((-3.14159265358979323846 / 2.0) + 0.0001);
    }
    void SetRot(const float p, const float y, const float r)
    {
        m_rot = MyMath::Vector3(p, y, r);
    }
    void SetPos(const float x, const float y, const float z) { m_pos = MyMath::Vector3(x, y, z); }
    const MyMath::Matrix GetInverseVMatrix() const { return m_inverse; }
    const MyMath::Matrix& GetPMatrix() const { return m_pMatrix; }
    const MyMath::Vector3& GetPos() const { return m_pos; }
    const MyMath::Vector3& GetRot() const { return m_rot; }
    float GetFarPlaneDistance() const { return m_far; }

private:
    void refresh()
    {
        rtx_params p;
        const float pos[3] = {m_pos.x, m_pos.y, m_pos.z}, rot[3] = {m_rot.x, m_rot.y, m_rot.z};
        if (rtx_camera_params(PrintMachine::GetWidth(), PrintMachine::GetHeight(), pos, rot, &p) != RTX_OK) {
            throw std::runtime_error("rtx_camera_params: singular view matrix or PrintMachine not started");
        }
        m_inverse = MyMath::Matrix(MyMath::Vector4(p.inv_v[0], p.inv_v[1], p.inv_v[2], p.inv_v[3]),
                                   MyMath::Vector4(p.inv_v[4], p.inv_v[5], p.inv_v[6], p.inv_v[7]),
                                   MyMath::Vector4(p.inv_v[8], p.inv_v[9], p.inv_v[10], p.inv_v[11]),
                                   MyMath::Vector4(p.inv_v[12], p.inv_v[13], p.inv_v[14], p.inv_v[15]));
        m_pMatrix.row1.x = p.element1;
        m_pMatrix.row2.y = p.element2;
        m_far = p.cam_far;
        // Camera3D.cpp:61-71
        const float yaw = m_rot.y;
        m_staticForward = MyMath::Vector3(-std::sin(yaw), -std::cos(yaw), -std::cos(yaw));
        m_staticRight = MyMath::Vector3(std::cos(yaw), -std::sin(yaw), -std::sin(yaw));
    }
    MyMath::Matrix m_inverse, m_pMatrix;
    MyMath::Vector3 m_staticForward, m_staticRight;
    MyMath::Vector3 m_pos;
    MyMath::Vector3 m_rot = MyMath::Vector3(0.0f, 3.14159274101257324f, 0.0f); // Camera3D.h:62
    float m_far = 250.0f;
};

// ---------------------------------------------------------------------------------------------
class RayTracing {
public:
    RayTracing() = delete;
    // params: HOST pointer here (device pointer in the reference); resultArray: device memory, pre-zeroed by
    // the caller as in the reference; gridDims/blockDims are accepted and ignored.
    static void RayTrace(const dim3_compat&, const dim3_compat&, Object3D** const objects, const unsigned int count,
                         const RayTracingCPUToGPUData* params, char* resultArray, const RenderingMode mode)
    {
        rtx_ctx* ctx = reinterpret_cast<rtx_ctx*>(objects);
        if (!ctx || !params) throw std::runtime_error("RayTracing::RayTrace: null scene handle or params");
        if (count != rtx_scene_count(ctx)) throw std::runtime_error("RayTracing::RayTrace: count does not match the scene");
        const rtx_params p = rtx_compat::to_rtx_params(*params);
        rtx_compat::check(ctx, rtx_render_rows(ctx, &p, (int)mode, 0, (size_t)p.y, resultArray, 0, nullptr, RTX_RENDER_DEFAULT),
                          "rtx_render_rows");
    }
};

// ---------------------------------------------------------------------------------------------
class RayTracingManager {
public:
    RayTracingManager()
    {
        // the constructor sizes its buffers from PrintMachine::GetMaxSize() (RayTracingManager.cu:58-66)
        if (PrintMachine::GetMaxSize() == 0) throw std::runtime_error("PrintMachine::Start must precede RayTracingManager()");
        m_ctx = rtx_compat::Device::get(PrintMachine::GetWidth(), PrintMachine::GetHeight());
        // pinned, so that the copy of the minimised stream runs at PCIe rate (the reference's is pageable)
        m_minimizedResultArray = static_cast<char*>(rtx_host_alloc(m_ctx, PrintMachine::GetMaxSize()));
        if (!m_minimizedResultArray) throw std::runtime_error(std::string("rtx_host_alloc: ") + rtx_last_error(m_ctx));
    }
    ~RayTracingManager()
    {
        // the shared context itself is released by PrintMachine::CleanUp()
        if (rtx_compat::Device::slot() == m_ctx) rtx_host_free(m_ctx, m_minimizedResultArray);
    }

    // Synchronous, like the reference: on return the minimised frame is in PrintMachine's back buffer.
    void Update(const RayTracingCPUToGPUData& params, const DeviceObjectArray<Object3D*>& deviceObjects, double dt)
    {
        if (reinterpret_cast<rtx_ctx*>(deviceObjects.m_deviceArray) != m_ctx) {
            throw std::runtime_error("RayTracingManager::Update: objects do not belong to this device context");
        }
        const rtx_params p = rtx_compat::to_rtx_params(params);
        size_t newSize = 0;
        if (m_halfDeltaFrames) {
            // two pixel rows per console row, and only the cells whose colours changed (rtx_update_half_delta): a key frame first, after
            // SetHalfDeltaFrames, and whenever the library decides on one; the printer appends deltas it has not written yet
            int kind = RTX_DELTA_KEY;
            const int rc = rtx_update_half_delta(m_ctx, &p, (int)currentRenderingMode, dt, /*run_physics=*/1, m_wantKey ? RTX_DELTA_KEYFRAME : RTX_DELTA_DEFAULT,
                                                 m_minimizedResultArray, PrintMachine::GetMaxSize(), &newSize, &kind);
            if (rc != RTX_ERR_TOO_LARGE) rtx_compat::check(m_ctx, rc, "rtx_update_half_delta");
            m_wantKey = false;
            if (rc == RTX_ERR_TOO_LARGE || !PrintMachine::SetDeltaInBackBuffer(m_minimizedResultArray, newSize, kind == RTX_DELTA_KEY)) {
                // a delta longer than the buffers (rtx_half_delta_bound is above rtx_half_bound), or unprinted deltas that have outgrown
                // the back buffer: the same frame once more (no physics), whole, replaces them
                rtx_compat::check(m_ctx, rtx_update_half_delta(m_ctx, &p, (int)currentRenderingMode, 0.0, /*run_physics=*/0, RTX_DELTA_KEYFRAME,
                                                               m_minimizedResultArray, PrintMachine::GetMaxSize(), &newSize, &kind), "rtx_update_half_delta");
                PrintMachine::SetDeltaInBackBuffer(m_minimizedResultArray, newSize, true);
            }
            return;
        }
        if (m_halfBlocks) {
            // two pixel rows per console row (rtx_update_half): a whole frame every time, handed over as rtx_update's is
            rtx_compat::check(m_ctx, rtx_update_half(m_ctx, &p, (int)currentRenderingMode, dt, /*run_physics=*/1, m_minimizedResultArray,
                                                     PrintMachine::GetMaxSize(), &newSize), "rtx_update_half");
            PrintMachine::SetDataInBackBuffer(m_minimizedResultArray, newSize);
            return;
        }
        if (m_deltaFrames) {
            // only the cells that changed (rtx_update_delta): a key frame first, after SetDeltaFrames, and whenever the library
            // decides on one (another size or mode); the printer appends deltas it has not written yet
            int kind = RTX_DELTA_KEY;
            rtx_compat::check(m_ctx, rtx_update_delta(m_ctx, &p, (int)currentRenderingMode, dt, /*run_physics=*/1, m_wantKey ? RTX_DELTA_KEYFRAME : RTX_DELTA_DEFAULT,
                                                      m_minimizedResultArray, PrintMachine::GetMaxSize(), &newSize, &kind), "rtx_update_delta");
            m_wantKey = false;
            if (!PrintMachine::SetDeltaInBackBuffer(m_minimizedResultArray, newSize, kind == RTX_DELTA_KEY)) {
                // the unprinted deltas have outgrown the back buffer: the same frame once more (no physics), whole, replaces them
                rtx_compat::check(m_ctx, rtx_update_delta(m_ctx, &p, (int)currentRenderingMode, 0.0, /*run_physics=*/0, RTX_DELTA_KEYFRAME,
                                                          m_minimizedResultArray, PrintMachine::GetMaxSize(), &newSize, &kind), "rtx_update_delta");
                PrintMachine::SetDeltaInBackBuffer(m_minimizedResultArray, newSize, true);
            }
            return;
        }
        rtx_compat::check(m_ctx, rtx_update(m_ctx, &p, (int)currentRenderingMode, dt, /*run_physics=*/1,
                                            m_minimizedResultArray, &newSize), "rtx_update");
        PrintMachine::SetDataInBackBuffer(m_minimizedResultArray, newSize);
    }
    // Extension, no reference counterpart (PrintMachine.cpp:257-306 rewrites the screen; RayTracingManager.cu:150 hands over whole
    // frames): Update sends only the console cells that changed since the frame before.  Off by default, and then nothing changes.
    void SetDeltaFrames(const bool on)
    {
        m_deltaFrames = on;
        m_wantKey = true;
        PrintMachine::SetDeltaMode(on);
    }
    // Extension, no reference counterpart (RayTracing.cu:256,476 paint one colour per cell): Update hands over half-block frames --
    // every cell the glyph U+2580 with the colour of pixel row 2r in front and that of row 2r + 1 behind, W x 2H square pixels on a
    // W x H console (rtx_update_half; the two PIXEL modes are what it is for, a UTF-8 terminal what it needs).  The printer's buffers
    // and the device context must have been made for it: PrintMachine::Start(x, y, true) first, else this throws.  While on, delta
    // frames (SetDeltaFrames) are ignored: every frame is whole (half-block frames have a delta form of their own,
    // SetHalfDeltaFrames); switching off makes the next delta frame a key frame.  Off by default, and then nothing changes.
    void SetHalfBlocks(const bool on)
    {
        if (on && !PrintMachine::HalfBlocks()) throw std::runtime_error("RayTracingManager::SetHalfBlocks: PrintMachine::Start(x, y, true) must come first");
        m_halfBlocks = on;
        m_wantKey = true;
    }
    // Extension, no reference counterpart (RayTracing.cu:256,476; PrintMachine.cpp:257-306; RayTracingManager.cu:150): Update hands over
    // half-block frames as SetHalfBlocks does, but after the first only the cells whose two colours changed, each run behind a cursor
    // escape (rtx_update_half_delta).  Needs PrintMachine::Start(x, y, true), as SetHalfBlocks does, else this throws; switches the
    // printer to delta mode.  While on it decides what Update sends, whatever SetHalfBlocks and SetDeltaFrames say; switching it off
    // leaves the printer's delta mode to SetDeltaFrames.  Off by default, and then nothing changes.
    void SetHalfDeltaFrames(const bool on)
    {
        if (on && !PrintMachine::HalfBlocks()) throw std::runtime_error("RayTracingManager::SetHalfDeltaFrames: PrintMachine::Start(x, y, true) must come first");
        m_halfDeltaFrames = on;
        m_wantKey = true;
        PrintMachine::SetDeltaMode(on || m_deltaFrames);
    }
    void SetRenderingMode(const RenderingMode newRenderMode) { currentRenderingMode = newRenderMode; }
    // Extensions, no reference counterpart (its light is a constant, RayTracing.cu:132,143-157): the point light (nullptr: the
    // reference's) and hard shadows (RTX_OPT_SHADOWS).
    void SetLight(const rtx_light* light) { rtx_compat::check(m_ctx, rtx_scene_set_light(m_ctx, light), "rtx_scene_set_light"); }
    void SetLights(const rtx_light* lights, const size_t n) { rtx_compat::check(m_ctx, rtx_scene_set_lights(m_ctx, n, lights), "rtx_scene_set_lights"); }
    // Extension, no reference counterpart (RayTracing.cu:132): a cone and a soft edge per light of the set (rtx_scene_set_spots: n the
    // number of lights, or 0 for point lights again).  SetLight and SetLights clear the cones: set the lights first.
    void SetSpots(const rtx_spot* spots, const size_t n) { rtx_compat::check(m_ctx, rtx_scene_set_spots(m_ctx, n, spots), "rtx_scene_set_spots"); }
    void SetShadows(const bool on) { rtx_compat::check(m_ctx, rtx_set_option(m_ctx, RTX_OPT_SHADOWS, on ? 1 : 0), "rtx_set_option(RTX_OPT_SHADOWS)"); }
    // Extension, no reference counterpart (RayTracing.cu:12-17 traces one ray per console cell): n x n rays per cell, n in 1 .. 4, folded
    // on the GPU (RTX_OPT_SUPERSAMPLE); Update then hands over the folded cells.  1 by default, and then nothing changes.
    void SetSupersampling(const int n) { rtx_compat::check(m_ctx, rtx_set_option(m_ctx, RTX_OPT_SUPERSAMPLE, n), "rtx_set_option(RTX_OPT_SUPERSAMPLE)"); }

private:
    rtx_ctx* m_ctx = nullptr;
    char* m_minimizedResultArray = nullptr;
    bool m_deltaFrames = false, m_wantKey = true; // SetDeltaFrames
    bool m_halfBlocks = false;                    // SetHalfBlocks
    bool m_halfDeltaFrames = false;               // SetHalfDeltaFrames
    RenderingMode currentRenderingMode = BIT_ASCII; // RayTracingManager.h:53
};
