/*
 * driver.cpp -- runs the reference's own sources, compiled for the host (see prefix.h), on one case file.
 *
 *     ref_driver CASE_FILE RESULT_FILE
 *
 * Test infrastructure: tests/ref_host.py writes the case, starts this program as a child process and parses the
 * result.  The formats are documented at the top of tests/ref_host.py.  Everything that computes is the
 * reference's: Scene3D::CreateSphere / CreatePlane / Init, Camera3D::SetPos / SetRot / Init / Update /
 * GetInverseVMatrix, RayTracingManager::Update (UpdateObjects, the RayTrace_* kernel, the copy back,
 * MinimizeResults), RayTracingManager::MinimizeResults alone, ansi256_from_rgb.  This file only moves bytes in
 * and out, and supplies the four PrintMachine functions those sources link against.
 */
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

/* RayTracing.cu's translation unit defines it (ANSIRGB.h:141); no header declares it. */
uint8_t ansi256_from_rgb(uint32_t rgb);

namespace {

size_t g_width = 0, g_height = 0;
std::vector<char> g_back_buffer; /* what RayTracingManager::Update hands to PrintMachine::SetDataInBackBuffer */

}  // namespace

/* PrintMachine: the console side of the reference is not built; these four are what the rest links against. */
size_t PrintMachine::GetWidth() { return g_width; }
size_t PrintMachine::GetHeight() { return g_height; }
size_t PrintMachine::GetMaxSize() { return 20 * g_width * g_height; }
void PrintMachine::SetDataInBackBuffer(const char* data, const size_t size) { g_back_buffer.assign(data, data + size); }

namespace {

enum Kind : uint32_t { KIND_UPDATE = 0, KIND_MINIMIZE = 1, KIND_ANSI256 = 2, KIND_CAMERA = 3 };
const uint32_t MAGIC = 0x43585452; /* "RTXC" */

struct ObjectRecord { /* 60 bytes, the oracle's orc_object */
    int32_t type;     /* 1 plane, 2 sphere (ObjectType, Object3D.h:14) */
    float center[3], color[3], radius;
    int32_t mover;
    float speed, normal[3], width, height;
};

struct Reader {
    std::vector<unsigned char> buf;
    size_t at = 0;
    void get(void* dst, size_t n)
    {
        if (at + n > buf.size()) {
            throw std::runtime_error("case file is truncated");
        }
        std::memcpy(dst, buf.data() + at, n);
        at += n;
    }
    uint32_t u32()
    {
        uint32_t v;
        get(&v, 4);
        return v;
    }
};

struct Writer {
    FILE* f;
    void put(const void* src, size_t n)
    {
        if (n && std::fwrite(src, 1, n, f) != n) {
            throw std::runtime_error("cannot write the result file");
        }
    }
    void u32(uint32_t v) { put(&v, 4); }
    void u64(uint64_t v) { put(&v, 8); }
};

void put_params(Writer& w, const RayTracingCPUToGPUData& p)
{
    const MyMath::Vector4* rows[4] = {&p.inverseVMatrix.row1, &p.inverseVMatrix.row2, &p.inverseVMatrix.row3, &p.inverseVMatrix.row4};
    float out[22];
    for (int i = 0; i < 4; i++) {
        out[4 * i + 0] = rows[i]->x;
        out[4 * i + 1] = rows[i]->y;
        out[4 * i + 2] = rows[i]->z;
        out[4 * i + 3] = rows[i]->w;
    }
    out[16] = p.camPos.x;
    out[17] = p.camPos.y;
    out[18] = p.camPos.z;
    out[19] = p.element1;
    out[20] = p.element2;
    out[21] = p.camFarDist;
    w.put(out, sizeof out);
}

/* The params as the engine fills them from its camera each frame (Engine3D.cpp:21-22, 84, 90-97). */
RayTracingCPUToGPUData params_from_camera(const float pos[3], const float rot[3])
{
    Camera3D camera;
    camera.SetPos(pos[0], pos[1], pos[2]);
    camera.SetRot(rot[0], rot[1], rot[2]);
    camera.Init();
    camera.Update();
    RayTracingCPUToGPUData p;
    p.inverseVMatrix = camera.GetInverseVMatrix();
    p.camPos = camera.GetPos();
    p.x = PrintMachine::GetWidth();
    p.y = PrintMachine::GetHeight();
    p.element1 = camera.GetPMatrix().row1.x;
    p.element2 = camera.GetPMatrix().row2.y;
    p.camFarDist = camera.GetFarPlaneDistance();
    return p;
}

RayTracingCPUToGPUData params_raw(const float v[22])
{
    RayTracingCPUToGPUData p;
    MyMath::Vector4* rows[4] = {&p.inverseVMatrix.row1, &p.inverseVMatrix.row2, &p.inverseVMatrix.row3, &p.inverseVMatrix.row4};
    for (int i = 0; i < 4; i++) {
        *rows[i] = MyMath::Vector4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
    }
    p.camPos = MyMath::Vector3(v[16], v[17], v[18]);
    p.x = PrintMachine::GetWidth();
    p.y = PrintMachine::GetHeight();
    p.element1 = v[19];
    p.element2 = v[20];
    p.camFarDist = v[21];
    return p;
}

/* The three arrays Scene3D::Init allocates (Scene3D.cpp:10-25), without the objects it then creates. */
void allocate_scene_arrays(Scene3D& scene)
{
    cudaMalloc(&scene.m_deviceObjects.m_deviceArray, 80);
    cudaMemset(scene.m_deviceObjects.m_deviceArray, 0, 80);
    scene.m_deviceObjects.allocatedBytes = 80;
    scene.m_deviceObjects.count = 0;
    cudaMalloc(&scene.m_devicePlanes.m_deviceArray, FIVE_MEGABYTES);
    cudaMemset(scene.m_devicePlanes.m_deviceArray, 0, FIVE_MEGABYTES);
    scene.m_devicePlanes.allocatedBytes = FIVE_MEGABYTES;
    scene.m_devicePlanes.count = 0;
    cudaMalloc(&scene.m_deviceSpheres.m_deviceArray, FIVE_MEGABYTES);
    cudaMemset(scene.m_deviceSpheres.m_deviceArray, 0, FIVE_MEGABYTES);
    scene.m_deviceSpheres.allocatedBytes = FIVE_MEGABYTES;
    scene.m_deviceSpheres.count = 0;
}

void run_update(Reader& in, Writer& out)
{
    const uint32_t W = in.u32(), H = in.u32(), mode = in.u32(), scene_src = in.u32(), params_src = in.u32(),
                   nobj = in.u32(), nsteps = in.u32();
    in.u32();
    float pv[22];
    in.get(pv, sizeof pv);
    std::vector<ObjectRecord> recs(nobj);
    in.get(recs.data(), nobj * sizeof(ObjectRecord));
    std::vector<double> dts(nsteps);
    in.get(dts.data(), nsteps * sizeof(double));

    g_width = W;
    g_height = H;
    Scene3D scene;
    if (scene_src == 1) {
        scene.Init();
    } else {
        allocate_scene_arrays(scene);
        for (const ObjectRecord& r : recs) {
            const MyMath::Vector3 center(r.center[0], r.center[1], r.center[2]), color(r.color[0], r.color[1], r.color[2]);
            if (r.type == (int32_t)ObjectType::SphereType) {
                scene.CreateSphere(r.radius, center, color);
            } else if (r.type == (int32_t)ObjectType::PlaneType) {
                scene.CreatePlane(center, MyMath::Vector3(r.normal[0], r.normal[1], r.normal[2]), color, r.width, r.height);
            } else {
                throw std::runtime_error("object record with an unknown type");
            }
        }
    }
    DeviceObjectArray<Object3D*> objects = scene.GetObjects();
    if (objects.count != nobj) {
        throw std::runtime_error("the scene holds another number of objects than the case lists");
    }
    /* Sphere's constructor draws speed from rand() (Sphere.cu:11-12): the case says what it is to be. */
    for (uint32_t i = 0; i < nobj; i++) {
        Object3D* o = objects.m_deviceArray[i];
        if ((int32_t)o->GetType() != recs[i].type) {
            throw std::runtime_error("object types of the scene and the case differ");
        }
        if (o->GetType() == ObjectType::SphereType) {
            static_cast<Sphere*>(o)->mover = recs[i].mover;
            static_cast<Sphere*>(o)->speed = recs[i].speed;
        }
    }

    const RayTracingCPUToGPUData params = params_src == 1 ? params_from_camera(pv, pv + 3) : params_raw(pv);
    RayTracingManager manager;
    manager.SetRenderingMode((RenderingMode)mode);

    out.u32(MAGIC);
    out.u32(W);
    out.u32(H);
    out.u32(nsteps);
    out.u32(nobj);
    out.u32(0);
    put_params(out, params);
    for (uint32_t s = 0; s < nsteps; s++) {
        g_back_buffer.clear();
        manager.Update(params, objects, dts[s]);
        for (uint32_t i = 0; i < nobj; i++) {
            Object3D* o = objects.m_deviceArray[i];
            const float y = o->m_center.y;
            const int32_t mover = o->GetType() == ObjectType::SphereType ? static_cast<Sphere*>(o)->mover : 0;
            out.put(&y, 4);
            out.put(&mover, 4);
        }
        out.put(manager.m_hostResultArray.get(), PrintMachine::GetMaxSize());
        out.u64(g_back_buffer.size());
        out.put(g_back_buffer.data(), g_back_buffer.size());
    }
    scene.CleanUp();
}

void run_minimize(Reader& in, Writer& out)
{
    const uint32_t W = in.u32(), H = in.u32(), mode = in.u32();
    in.u32();
    g_width = W;
    g_height = H;
    RayTracingManager manager;
    manager.SetRenderingMode((RenderingMode)mode);
    const size_t size = PrintMachine::GetMaxSize();
    in.get(manager.m_hostResultArray.get(), size);
    const size_t n = manager.MinimizeResults(size, W, H);
    out.u32(MAGIC);
    out.u32(0);
    out.u64(n);
    out.put(manager.m_minimizedResultArray.get(), n);
}

void run_ansi256(Writer& out)
{
    std::vector<uint8_t> table(1u << 24);
    for (uint32_t rgb = 0; rgb < (1u << 24); rgb++) {
        table[rgb] = ansi256_from_rgb(rgb);
    }
    out.put(table.data(), table.size());
}

void run_camera(Reader& in, Writer& out)
{
    const uint32_t W = in.u32(), H = in.u32(), n = in.u32();
    in.u32();
    g_width = W;
    g_height = H;
    for (uint32_t i = 0; i < n; i++) {
        float pr[6];
        in.get(pr, sizeof pr);
        put_params(out, params_from_camera(pr, pr + 3));
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s CASE_FILE RESULT_FILE\n", argv[0]);
        return 2;
    }
    try {
        Reader in;
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) {
            throw std::runtime_error(std::string("cannot open ") + argv[1]);
        }
        unsigned char chunk[1 << 16];
        size_t n;
        while ((n = std::fread(chunk, 1, sizeof chunk, f)) > 0) {
            in.buf.insert(in.buf.end(), chunk, chunk + n);
        }
        std::fclose(f);
        if (in.u32() != MAGIC) {
            throw std::runtime_error("not a case file");
        }
        const uint32_t kind = in.u32();
        Writer out{std::fopen(argv[2], "wb")};
        if (!out.f) {
            throw std::runtime_error(std::string("cannot create ") + argv[2]);
        }
        switch (kind) {
        case KIND_UPDATE:
            run_update(in, out);
            break;
        case KIND_MINIMIZE:
            run_minimize(in, out);
            break;
        case KIND_ANSI256:
            run_ansi256(out);
            break;
        case KIND_CAMERA:
            run_camera(in, out);
            break;
        default:
            throw std::runtime_error("unknown case kind");
        }
        if (std::fclose(out.f) != 0) {
            throw std::runtime_error("cannot write the result file");
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ref_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
