// Scene3D::RemoveObject / RemoveObjects of include/rtx_compat.hpp: the facade renumbers the plane indices it holds by the rule of
// rtx_scene_remove_objects.  Needs a GPU (the facade owns a context); tests/test_gpu_compat_remove.py builds and runs it.
#include "rtx_compat.hpp"

#include <cstdio>

static int g_failed = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                 \
        }                                                               \
    } while (0)

static float k_of(rtx_ctx* ctx, unsigned i)
{
    float k = -1.0f;
    CHECK(rtx_scene_get_reflectivity(ctx, i, &k) == RTX_OK);
    return k;
}

int main()
{
    try {
        PrintMachine::Start(64, 24);
        rtx_ctx* ctx = rtx_compat::Device::get(PrintMachine::GetWidth(), PrintMachine::GetHeight());
        Scene3D scene;
        scene.CleanUp();
        const MyMath::Vector3 up(0.0f, 1.0f, 0.0f), grey(100.0f, 100.0f, 100.0f);
        scene.CreatePlane(MyMath::Vector3(0.0f, -3.0f, 30.0f), up, grey, 10, 20);   // object 0
        scene.CreateSphere(4.0f, MyMath::Vector3(0.0f, 5.0f, 30.0f), grey);          // object 1
        scene.CreatePlane(MyMath::Vector3(0.0f, -9.0f, 30.0f), up, grey, 30, 30);   // object 2
        scene.CreateSphere(2.0f, MyMath::Vector3(5.0f, 5.0f, 30.0f), grey);          // object 3
        scene.RemoveObject(0); // the first plane: sphere 0, plane 1, sphere 2 are left
        CHECK(rtx_scene_count(ctx) == 3);
        scene.SetPlaneReflectivity(0.5f); // the one plane the facade still holds, under its new index
        CHECK(k_of(ctx, 0) == 0.0f && k_of(ctx, 1) == 0.5f && k_of(ctx, 2) == 0.0f);
        int type = 0;
        float v[11];
        CHECK(rtx_scene_get_object(ctx, 1, &type, v) == RTX_OK && type == 1 && v[1] == -9.0f);
        scene.CreatePlane(MyMath::Vector3(0.0f, 20.0f, 30.0f), MyMath::Vector3(0.0f, -1.0f, 0.0f), grey, 30, 30); // object 3
        const unsigned gone[2] = {2u, 0u}; // both spheres, listed backwards: planes 0 and 1 are left
        scene.RemoveObjects(2, gone);
        CHECK(rtx_scene_count(ctx) == 2);
        scene.SetPlaneReflectivity(0.25f);
        CHECK(k_of(ctx, 0) == 0.25f && k_of(ctx, 1) == 0.25f);
        bool refused = false;
        try {
            scene.RemoveObject(2); // past the count: refused, and the facade's books stay
        } catch (const std::exception&) {
            refused = true;
        }
        CHECK(refused && rtx_scene_count(ctx) == 2);
        scene.SetPlaneReflectivity(0.75f);
        CHECK(k_of(ctx, 0) == 0.75f && k_of(ctx, 1) == 0.75f);
        PrintMachine::CleanUp();
    } catch (const std::exception& e) {
        std::printf("FAIL: %s\n", e.what());
        return 1;
    }
    if (g_failed) return 1;
    std::printf("facade removal ok\n");
    return 0;
}
