// rtx_lights_kernels.inc -- the shading launch for a set of several point lights (rtx_scene_set_lights), included into namespace
// rtx of rtx_kernels.hip after rtx_tile_pass.inc, which holds the device functions the tile passes share.  A set of one light
// keeps rtx_shadow_shade / rtx_reflect_shade (rtx_shadow_kernels.inc); these kernels take a set of two or more (or any set under
// RTX_OPT_LIGHTS_CHECK 1).  The launches before them are the same: the trace kernel in its kOutHit form and, on the mirror path,
// rtx_reflect_hit, which does not know about lights.
//
// The colour of a visible pixel: res = 0.2f * od; for each light in the order given res = (res + diffuse_i * od) + specular_i * 1.0f;
// res * 255.0f, minf(255.0f, .) -- shade_light's expression (rtx_device.hpp) with the per-light terms summed, every operation
// rounded to fp32, and for one light shade_light's operation for operation.  What does not depend on the light (point, view
// direction, nn) is formed once.  A light the pixel is shadowed from enters with both powers 0.
//
// The shadow test per light is the one-light pass's: self-shadow, the planes per pixel (shadowed_before_spheres), then the spheres.
// It is lights_dark_set (rtx_tile_pass.inc), which rtx_chain_shadow (rtx_chain_shadow_kernels.inc) runs over the deeper levels'
// hit points: every thread keeps a bit mask of the lights still open for its pixel.  Per light the workgroup reduces its open hit
// points to a cone from that light (light_cone), kept in LDS; a light with no open pixel in the workgroup has no cone.  The sphere
// array is then walked ONCE for all lights (walk_spheres): each staged sphere is tested against every live cone and, if kept for at
// least one light, appended once to the LDS list with the 8-bit mask of the lights it was kept for.  At a flush every wave goes
// through the lights some lane of it is still open for; per light the segment (toL, 1 / len2) is formed once and the list entries
// whose mask names the light (four mask bytes a word) are tested by the lanes open for it (segment_hits_sphere).

// (rtx_tile_pass.inc: LightsShared, the workgroup's LDS)

// diffuse_i and specular_i of one light, as shade_light forms them; res = (res + diffuse_i * od) + specular_i * 1.0f
__device__ __forceinline__ void add_light(V3& res, V3 point, V3 nn, V3 nv, V3 od, const rtxlights::PackedLight& L, float dpow, float spow)
{
    V3 lightDir = sub(v3(L.px, L.py, L.pz), point);
    float dist = sqrt_cr(lightDir.x * lightDir.x + lightDir.y * lightDir.y + lightDir.z * lightDir.z);
    dist = dist * dist;
    const float divDistance = rcp_cr(dist);
    lightDir = normalize_gpu(lightDir);

    const float diffuseIntensity = clampf(dot(nn, lightDir), 0.0f, 1.0f);
    const V3 diffuse = v3(((L.dr * diffuseIntensity) * dpow) * divDistance, ((L.dg * diffuseIntensity) * dpow) * divDistance,
                          ((L.db * diffuseIntensity) * dpow) * divDistance);

    const V3 h = normalize_gpu(add(lightDir, nv));
    const float specularIntensity = pow32(clampf(dot(nn, h), 0.0f, 1.0f));
    const V3 specular = v3(((L.sr * specularIntensity) * spow) * divDistance, ((L.sg * specularIntensity) * spow) * divDistance,
                           ((L.sb * specularIntensity) * spow) * divDistance);

    res.x = (res.x + diffuse.x * od.x) + specular.x * 1.0f;
    res.y = (res.y + diffuse.y * od.y) + specular.y * 1.0f;
    res.z = (res.z + diffuse.z * od.z) + specular.z * 1.0f;
}

// shade_light over the set: bit i of `shadowed` puts light i in with both powers 0.
__device__ __forceinline__ V3 shade_lights(const Ray& r, float distance, V3 normal, V3 od, const rtxlights::Block& ls, uint32_t shadowed)
{
    const V3 point = add(r.o, mulf(r.d, distance));
    const V3 viewDir = normalize_gpu(mulf(r.d, -1.0f));
    const V3 nn = normalize_gpu(normal);
    const V3 nv = normalize_gpu(viewDir);
    V3 res = v3(0.2f * od.x, 0.2f * od.y, 0.2f * od.z);
    for (uint32_t i = 0; i < ls.n; i++) {
        const bool dark = ((shadowed >> i) & 1u) != 0u;
        add_light(res, point, nn, nv, od, ls.light[i], dark ? 0.0f : ls.light[i].dpow, dark ? 0.0f : ls.light[i].spow);
    }
    res = mulf(res, 255.0f);
    return v3(minf(255.0f, res.x), minf(255.0f, res.y), minf(255.0f, res.z));
}

// add_light for an object with a finish (rtx_scene_set_finish; the rule: rtx_finish.hpp): kd and ks where add_light has no factor
// and 1.0f, the 2^m-th power where it has pow32.  The light's cone (rtx_scene_set_spots; the rule: rtx_spot.hpp): both powers
// times w, which is exactly 1 for a point light.
__device__ __forceinline__ void add_light(V3& res, V3 point, V3 nn, V3 nv, V3 od, const rtxlights::PackedLight& L, float dpow, float spow, const rtx_finish& f,
                                          const rtxspot::Packed& sp)
{
    V3 lightDir = sub(v3(L.px, L.py, L.pz), point);
    float dist = sqrt_cr(lightDir.x * lightDir.x + lightDir.y * lightDir.y + lightDir.z * lightDir.z);
    dist = dist * dist;
    const float divDistance = rcp_cr(dist);
    lightDir = normalize_gpu(lightDir);
    const float w = rtxspot::weight(sp, lightDir.x, lightDir.y, lightDir.z);
    dpow = dpow * w;
    spow = spow * w;

    const float diffuseIntensity = clampf(dot(nn, lightDir), 0.0f, 1.0f);
    const V3 diffuse = v3(((L.dr * diffuseIntensity) * dpow) * divDistance, ((L.dg * diffuseIntensity) * dpow) * divDistance,
                          ((L.db * diffuseIntensity) * dpow) * divDistance);

    const V3 h = normalize_gpu(add(lightDir, nv));
    const float specularIntensity = rtxfinish::power(clampf(dot(nn, h), 0.0f, 1.0f), f.shininess_log2);
    const V3 specular = v3(((L.sr * specularIntensity) * spow) * divDistance, ((L.sg * specularIntensity) * spow) * divDistance,
                           ((L.sb * specularIntensity) * spow) * divDistance);

    res.x = rtxfinish::add_terms(res.x, diffuse.x, f.diffuse, od.x, specular.x, f.specular);
    res.y = rtxfinish::add_terms(res.y, diffuse.y, f.diffuse, od.y, specular.y, f.specular);
    res.z = rtxfinish::add_terms(res.z, diffuse.z, f.diffuse, od.z, specular.z, f.specular);
}

// shade_lights for an object with a finish, under lights with cones.
__device__ __forceinline__ V3 shade_lights(const Ray& r, float distance, V3 normal, V3 od, const rtxlights::Block& ls, uint32_t shadowed, const rtx_finish& f,
                                           const rtxspot::Block& sp)
{
    const V3 point = add(r.o, mulf(r.d, distance));
    const V3 viewDir = normalize_gpu(mulf(r.d, -1.0f));
    const V3 nn = normalize_gpu(normal);
    const V3 nv = normalize_gpu(viewDir);
    V3 res = v3(rtxfinish::ambient(f.ambient, od.x), rtxfinish::ambient(f.ambient, od.y), rtxfinish::ambient(f.ambient, od.z));
    for (uint32_t i = 0; i < ls.n; i++) {
        const bool dark = ((shadowed >> i) & 1u) != 0u;
        add_light(res, point, nn, nv, od, ls.light[i], dark ? 0.0f : ls.light[i].dpow, dark ? 0.0f : ls.light[i].spow, f, sp.spot[i]);
    }
    res = mulf(res, 255.0f);
    return v3(minf(255.0f, res.x), minf(255.0f, res.y), minf(255.0f, res.z));
}

// FIN (rtx_scene_set_finish, rtx_scene_set_spots: the forms launched while some object has a finish of its own or some light a
// cone): every shade_lights takes the finish of the object it shades and the cones of the set (la is a SpotLightsArgs); without,
// nothing of either is compiled and the code is what it was before there were finishes and cones.
template <bool FIN, class LA>
__device__ __forceinline__ V3 shade_lights_of(const PatternArgs& pa, uint32_t id, const Ray& r, float distance, V3 normal, V3 od, const LA& la, uint32_t shadowed)
{
    if constexpr (FIN) {
        return shade_lights(r, distance, normal, od, la.lights, shadowed, finish_of(pa, id), la.spots);
    } else {
        return shade_lights(r, distance, normal, od, la.lights, shadowed);
    }
}

// (rtx_lights_chain_kernels.inc: the blend over a chain of up to RTX_MAX_REFLECT_DEPTH levels; deep_dark: byte j - 1 the lights
// level j is shadowed from)
template <bool FIN>
__device__ __forceinline__ V3 lights_chain_blend_dark(const KArgs& a, const LightsArgsOf<FIN>& la, const ReflectArgs& ra, const ChainArgs& ca, const PatternArgs& pa,
                                                      const Ray& ray, float distance, V3 normal, uint32_t id, V3 cl, size_t at, uint32_t deep_dark);
template <bool FIN>
__device__ __forceinline__ V3 lights_chain_blend(const KArgs& a, const LightsArgsOf<FIN>& la, const ReflectArgs& ra, const ChainArgs& ca, const PatternArgs& pa,
                                                 const Ray& ray, float distance, V3 normal, uint32_t id, V3 cl, size_t at);

// What the shade family of the grid path keeps of LightsShared (RTX_OPT_SHADOW_GRID, rtx_grid_shadow_kernels.inc): the encoder's tables.
struct ShadeTablesShared {
    uint32_t digits[256];
    __attribute__((aligned(4))) uint8_t ramp[68];
};

// REFLECT 0: no mirror; 1: one bounce (ra.hits2, reflect_blend with every light at full powers); 2: a chain (ca,
// lights_chain_blend); 3: a chain whose deeper levels were shadow-tested (RTX_OPT_REFLECT_SHADOWS: deep_dark, the words
// rtx_chain_shadow left, laid out as the hits).  DARK0: level 0's dark set is read from dark0 (a word per pixel, laid out as the
// hits: rtx_grid_shadow's output) instead of computed here -- no cone, no walk, no list in LDS.  What a value does not use is not
// compiled.  FIN: the objects' finishes are read (shade_lights_of).
template <int MODE, int OUT, int REFLECT, bool DARK0 = false, bool FIN = false>
__device__ __forceinline__ void lights_shade_body(const KArgs& a, const LightsArgsOf<FIN>& la, const ReflectArgs& ra, const ChainArgs& ca, const PatternArgs& pa,
                                                  const uint32_t* deep_dark = nullptr, const uint32_t* dark0 = nullptr)
{
    __shared__ std::conditional_t<DARK0, ShadeTablesShared, LightsShared> s;

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = tid >> 6;
    s.digits[tid] = digits_word(tid);
    if (tid < 17u) {
        reinterpret_cast<uint32_t*>(s.ramp)[tid] = reinterpret_cast<const uint32_t*>(kRamp)[tid];
    }
    if constexpr (!DARK0) {
        if (tid == 0u) s.cnt = 0u; // (these three: visible behind the first light's first barrier)
    }

    const Camera cam = tile_camera(a);
    const TilePixel px = tile_pixel(a, cam, la.hits, tid);
    const Ray& ray = px.ray;

    // the winner's normal and colour
    const uint32_t id = px.hit.y;
    const bool any_hit = px.in_frame && !px.newline_col && id != 0xffffffffu;
    float distance = kNoHit, shadingValue = 0.0f;
    V3 normal = ray.d, colour = ray.d, od = ray.d;
    if (any_hit) {
        distance = __uint_as_float(px.hit.x);
        const Surface sf = surface_of(a, pa, id, add(ray.o, mulf(ray.d, distance)));
        normal = sf.normal;
        od = sf.od;
        shadingValue = normal.x * 1.0f + normal.y * 0.0f + normal.z * 0.0f; // RayTracing.cu:133
    }

    // ---- the shadow test: per light self-shadow, planes and the workgroup's cone, then one walk of the scene for all lights
    const V3 P = add(ray.o, mulf(ray.d, distance)); // the point shade() lights
    const bool testable = la.test != 0u && any_hit && distance <= cam.far;
    uint32_t dark; // lights this pixel is shadowed from
    if constexpr (DARK0) {
        dark = testable ? dark0[px.at(a)] : 0u;
        lds_barrier(); // the encoder's tables are visible
    } else {
        dark = lights_dark_set(a, la, s, tid, lane, wave, P, normal, id, testable);
    }

    // ---- shade with every light (both powers 0 for the lights the pixel is shadowed from) and encode
    if (any_hit) {
        colour = shade_lights_of<FIN>(pa, id, ray, distance, normal, od, la, dark);
        if constexpr (REFLECT == 1) {
            if (distance <= cam.far) {
                colour = reflect_blend(a, ra, pa, ray, distance, normal, id, colour, px.at(a),
                                       [&](const Ray& r2, float t2, V3 n2, V3 od2, uint32_t id2) { return shade_lights_of<FIN>(pa, id2, r2, t2, n2, od2, la, 0u); });
            }
        } else if constexpr (REFLECT == 2) {
            if (distance <= cam.far) colour = lights_chain_blend<FIN>(a, la, ra, ca, pa, ray, distance, normal, id, colour, px.at(a));
        } else if constexpr (REFLECT == 3) {
            if (distance <= cam.far) colour = lights_chain_blend_dark<FIN>(a, la, ra, ca, pa, ray, distance, normal, id, colour, px.at(a), deep_dark[px.at(a)]);
        }
    }
    encode_and_store<MODE, OUT>(a, cam, s.digits, s.ramp, px.in_frame, px.newline_col, px.row, px.col, distance, normal, colour, shadingValue);
}

template <int MODE, int OUT, bool FIN = false>
__global__ __launch_bounds__(kThreads) void rtx_lights_shade(const KArgs a, const LightsArgsOf<FIN> la, const PatternArgs pa)
{
    const ReflectArgs ra = {}; // (read only by the REFLECT parts, which are not compiled here)
    const ChainArgs ca = {};
    lights_shade_body<MODE, OUT, 0, false, FIN>(a, la, ra, ca, pa);
}

// The mirror path's third launch for a set of several lights: rtx_lights_shade's shading, then the blend.
template <int MODE, int OUT, bool FIN = false>
__global__ __launch_bounds__(kThreads) void rtx_lights_reflect_shade(const KArgs a, const LightsArgsOf<FIN> la, const ReflectArgs ra, const PatternArgs pa)
{
    const ChainArgs ca = {}; // (read only by the chain's blend, which is not compiled here)
    lights_shade_body<MODE, OUT, 1, false, FIN>(a, la, ra, ca, pa);
}
