// tile_check.hip -- TEST INFRASTRUCTURE (built by __graft_entry__.build(), loaded only by tests/test_gpu_tile_bound.py).
// Runs the tile passes' culling -- light_cone, build_bundles, walk_spheres, lights_dark_set of rtx_tile_pass.inc with
// rtxshadow::may_occlude and rtxreflect::may_hit: the very text rtx_kernels.hip compiles -- on tiles of the caller's making, one
// 256-thread workgroup per tile, blockIdx.x the tile, and hands back what the device held: the cone as every thread has it, the
// bundles, every filling of the LDS list as the flush saw it, the threads' verdicts.  Beside them the production exact tests
// (segment_hits_sphere, secondary_sphere_hit) and the two keep conditions on pairs of the caller's choosing.
//
// A tile is 8 words (sph_off, ns, np, brute, light_off, nl, rec_off, rec_cap): its spheres are sph[sph_off .. sph_off + ns), known
// by position in that range; its planes the first np of the call's; its lights lights[light_off .. light_off + nl) (the cone and
// the shadow walk use the first); its list record rec[rec_off .. rec_off + rec_cap), 8 words an entry (position, the float4 read
// from the list, payload byte, filling number, slot in the list).  Per thread, npts <= 256 of them a tile: flags (bit 0: pending
// / testable), a point P, a normal N, an object id (sphere position, or plane index | bit 31), a secondary ray (O, D).  Threads
// from npts on are idle.  Every entry point returns 0, -1 on a HIP error, -2 on arguments it refuses (nothing is launched).
//
// lights_dark_set's flush is a lambda inside the function: it cannot be swapped for a recording one without editing production
// text, so the dark set returns `dark` and `longest` alone.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_cull.hpp"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_reflect.hpp"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_shadow.hpp"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_workgroup.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace rtx {
#include "../../raytracing-in-windows-console_amd/csrc/rtx_tile_pass.inc"
} // namespace rtx

namespace {

using namespace rtx;

constexpr uint32_t kTileWords = 8, kRecWords = 8, kConeWords = 7, kBundleWords = 10;

struct Tile {
    uint32_t sph_off, ns, np, brute, light_off, nl, rec_off, rec_cap;
};

// The call's arrays, on the host as the caller passes them and on the device as the kernels read them.
struct TileIn {
    const Tile* tiles;
    uint32_t ntiles, npts;
    const uint32_t* flags; // ntiles * npts
    const float* P;        // ... * 3
    const float* N;
    const uint32_t* id;
    const float* O;
    const float* D;
    const float4* sph_geom; // nsph
    const float4* sph_od;
    uint32_t nsph;
    const float4* pl_a; // npl
    const float4* pl_b;
    const float4* pl_od;
    uint32_t npl;
    const float* lights; // nlights * 3
    uint32_t nlights;
};

struct TileOut {
    uint32_t* verdict; // ntiles * 256: light_cone's return value
    uint32_t* cone;    // ntiles * 256 * 7: ax ay az theta dmax slack all, as the thread holds them (zeros without a cone)
    uint32_t* flag;    // ntiles * 256: shadowed / dark
    uint32_t* hit;     // ntiles * 256 * 2: bt, bid
    uint32_t* nb;      // ntiles * 256: build_bundles' return value
    uint32_t* bundle;  // ntiles * 4 * 10: ox oy oz rho ax ay az theta slack all
    uint32_t* longest; // ntiles
    uint32_t* nfill;   // ntiles: flushes that found an entry
    uint32_t* rec_n;   // ntiles: entries over all fillings (those past rec_cap are counted, not recorded)
    uint32_t* rec;     // nrec * 8
    uint32_t nrec;
};

struct Thread {
    uint32_t tid, lane, wave;
    bool pending;
    V3 P, N;
    uint32_t id;
    Ray r;
};

__device__ __forceinline__ KArgs args_of(const TileIn& in, const Tile& t)
{
    KArgs a = {};
    a.ns = t.ns;
    a.sph_geom = in.sph_geom + t.sph_off;
    a.sph_od = in.sph_od + t.sph_off;
    a.np = t.np;
    a.pl_a = in.pl_a;
    a.pl_b = in.pl_b;
    a.pl_od = in.pl_od;
    return a;
}

__device__ __forceinline__ Thread thread_of(const TileIn& in, uint32_t tile)
{
    Thread th;
    th.tid = threadIdx.x;
    th.lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    th.wave = th.tid >> 6;
    th.pending = false;
    th.P = th.N = v3(0.0f, 0.0f, 0.0f);
    th.id = 0xffffffffu;
    th.r.o = th.r.d = v3(0.0f, 0.0f, 0.0f);
    if (th.tid < in.npts) {
        const size_t k = (size_t)tile * in.npts + th.tid;
        th.pending = (in.flags[k] & 1u) != 0u;
        if (in.P) th.P = v3(in.P[3 * k], in.P[3 * k + 1], in.P[3 * k + 2]);
        if (in.N) th.N = v3(in.N[3 * k], in.N[3 * k + 1], in.N[3 * k + 2]);
        if (in.id) th.id = in.id[k];
        if (in.O) th.r.o = v3(in.O[3 * k], in.O[3 * k + 1], in.O[3 * k + 2]);
        if (in.D) th.r.d = v3(in.D[3 * k], in.D[3 * k + 1], in.D[3 * k + 2]);
    }
    // rtx_tile_pass.inc (mirror_ray): a = R . R, fourA = 4a, divTwoA = 1 / (2a)
    th.r.a = dot(th.r.d, th.r.d);
    th.r.fourA = 4.0f * th.r.a;
    th.r.divTwoA = rcp_cr(2.0f * th.r.a);
    return th;
}

__device__ __forceinline__ void put_cone(uint32_t* o, const rtxshadow::Cone& c, bool have)
{
    o[0] = have ? __float_as_uint(c.ax) : 0u;
    o[1] = have ? __float_as_uint(c.ay) : 0u;
    o[2] = have ? __float_as_uint(c.az) : 0u;
    o[3] = have ? __float_as_uint(c.theta) : 0u;
    o[4] = have ? __float_as_uint(c.dmax) : 0u;
    o[5] = have ? __float_as_uint(c.slack) : 0u;
    o[6] = have && c.all ? 1u : 0u;
}

__device__ __forceinline__ void put_bundle(uint32_t* o, const rtxreflect::Bundle& b)
{
    o[0] = __float_as_uint(b.ox);
    o[1] = __float_as_uint(b.oy);
    o[2] = __float_as_uint(b.oz);
    o[3] = __float_as_uint(b.rho);
    o[4] = __float_as_uint(b.ax);
    o[5] = __float_as_uint(b.ay);
    o[6] = __float_as_uint(b.az);
    o[7] = __float_as_uint(b.theta);
    o[8] = __float_as_uint(b.slack);
    o[9] = b.all ? 1u : 0u;
}

// What a flush does besides the exact tests: the cnt entries of this filling, as the list holds them, to the tile's record.
// No barrier; `done` and `fills` are workgroup-uniform (cnt is).
__device__ __forceinline__ void record_filling(const TileOut& out, const Tile& t, uint32_t tid, const float4* s_list, const uint32_t* s_pos,
                                               const uint8_t* s_payload, uint32_t cnt, uint32_t& done, uint32_t& fills)
{
    for (uint32_t j = tid; j < cnt; j += (uint32_t)kThreads) {
        const uint32_t e = done + j;
        if (j < (uint32_t)kTileList && e < t.rec_cap && (size_t)t.rec_off + e < out.nrec) {
            uint32_t* o = out.rec + (size_t)kRecWords * (t.rec_off + e);
            const float4 g = s_list[j];
            o[0] = s_pos[j];
            o[1] = __float_as_uint(g.x);
            o[2] = __float_as_uint(g.y);
            o[3] = __float_as_uint(g.z);
            o[4] = __float_as_uint(g.w);
            o[5] = s_payload != nullptr ? (uint32_t)s_payload[j] : 0u;
            o[6] = fills;
            o[7] = j;
        }
    }
    done += cnt;
    fills += cnt != 0u ? 1u : 0u;
}

// light_cone alone: its verdict and the cone, from every thread.
__global__ __launch_bounds__(kThreads) void k_cone(TileIn in, TileOut out)
{
    __shared__ float s_red[4][6];
    const uint32_t tile = blockIdx.x;
    const Tile t = in.tiles[tile];
    const Thread th = thread_of(in, tile);
    const float Lf[3] = {in.lights[3 * t.light_off], in.lights[3 * t.light_off + 1], in.lights[3 * t.light_off + 2]};
    const float Pf[3] = {th.P.x, th.P.y, th.P.z};
    rtxshadow::Cone cone = {};
    const bool have = light_cone(Lf, Pf, th.pending, t.brute != 0u, t.ns, th.lane, th.wave, s_red, cone);
    const size_t k = (size_t)tile * kThreads + th.tid;
    out.verdict[k] = have ? 1u : 0u;
    put_cone(out.cone + kConeWords * k, cone, have);
}

// rtx_shadow_shade's sphere test (rtx_shadow_kernels.inc: shade_body, from light_cone on), the flush recording besides.
__global__ __launch_bounds__(kThreads) void k_shadow_walk(TileIn in, TileOut out)
{
    __shared__ float4 s_occ[kTileList];
    __shared__ uint32_t s_occ_pos[kTileList];
    __shared__ float s_red[4][6];
    __shared__ uint32_t s_cnt;

    const uint32_t tile = blockIdx.x;
    const Tile t = in.tiles[tile];
    const KArgs a = args_of(in, t);
    const Thread th = thread_of(in, tile);
    const uint32_t tid = th.tid, lane = th.lane, wave = th.wave, id = th.id;
    if (tid == 0u) s_cnt = 0u; // (visible behind light_cone's first barrier)

    const V3 L = v3(in.lights[3 * t.light_off], in.lights[3 * t.light_off + 1], in.lights[3 * t.light_off + 2]);
    const V3 P = th.P;
    const V3 toL = sub(L, P);
    bool pending = th.pending;
    bool shadowed = false;
    uint32_t done = 0u, fills = 0u;

    const float Lf[3] = {L.x, L.y, L.z};
    const float Pf[3] = {P.x, P.y, P.z};
    rtxshadow::Cone cone = {};
    const bool have = light_cone(Lf, Pf, pending, t.brute != 0u, a.ns, lane, wave, s_red, cone);
    if (have) {
        const float len2 = dot(toL, toL);
        const float inv_len2 = len2 > 0.0f ? 1.0f / len2 : 0.0f;
        const uint32_t own_sphere = (id & 0x80000000u) ? 0xffffffffu : id;
        walk_spheres<kTileList>(
            a, tid, lane, s_occ, s_occ_pos, nullptr, &s_cnt, out.longest + tile,
            [&](bool in0, float4 c0, bool in1, float4 c1, uint32_t& k0, uint32_t& k1) {
                k0 = in0 && rtxshadow::may_occlude(cone, Lf, c0.x, c0.y, c0.z, c0.w) ? 1u : 0u;
                k1 = in1 && rtxshadow::may_occlude(cone, Lf, c1.x, c1.y, c1.z, c1.w) ? 1u : 0u;
            },
            [&](uint32_t cnt) {
                record_filling(out, t, tid, s_occ, s_occ_pos, nullptr, cnt, done, fills);
                for (uint32_t j = 0; j < cnt && __ballot(pending) != 0ull; j++) {
                    const float4 sp = s_occ[j];
                    if (pending && s_occ_pos[j] != own_sphere && segment_hits_sphere(P, toL, inv_len2, sp)) {
                        shadowed = true;
                        pending = false;
                    }
                }
            });
    }
    const size_t k = (size_t)tile * kThreads + tid;
    out.verdict[k] = have ? 1u : 0u;
    put_cone(out.cone + kConeWords * k, cone, have);
    out.flag[k] = shadowed ? 1u : 0u;
    if (tid == 0u) {
        out.nfill[tile] = fills;
        out.rec_n[tile] = done;
    }
}

// lights_dark_set, as lights_shade_body calls it.
__global__ __launch_bounds__(kThreads) void k_dark_set(TileIn in, TileOut out)
{
    __shared__ LightsShared s;
    const uint32_t tile = blockIdx.x;
    const Tile t = in.tiles[tile];
    const KArgs a = args_of(in, t);
    const Thread th = thread_of(in, tile);
    if (th.tid == 0u) s.cnt = 0u; // (visible behind the first light's first barrier)
    LightsArgs la = {};
    la.lights.n = t.nl;
    for (uint32_t i = 0; i < t.nl; i++) {
        la.lights.light[i].px = in.lights[3 * (t.light_off + i)];
        la.lights.light[i].py = in.lights[3 * (t.light_off + i) + 1];
        la.lights.light[i].pz = in.lights[3 * (t.light_off + i) + 2];
    }
    la.test = 1u;
    la.brute = t.brute;
    la.longest = out.longest + tile;
    const uint32_t dark = lights_dark_set(a, la, s, th.tid, th.lane, th.wave, th.P, th.N, th.id, th.pending);
    out.flag[(size_t)tile * kThreads + th.tid] = dark;
}

// build_bundles alone, and with MODE 1 rtx_reflect_hit's walk (rtx_reflect_kernels.inc, from closest_of_planes on), the flush
// recording besides.
template <int WALK>
__global__ __launch_bounds__(kThreads) void k_mirror(TileIn in, TileOut out)
{
    __shared__ float4 s_cand[WALK ? kTileList : 1];
    __shared__ uint32_t s_cand_pos[WALK ? kTileList : 1];
    __shared__ float s_red[4][8];
    __shared__ rtxreflect::Bundle s_bundle[kReflectBundles];
    __shared__ float s_lead_u[4][3];
    __shared__ uint32_t s_lead_lane[4];
    __shared__ uint32_t s_cnt;

    const uint32_t tile = blockIdx.x;
    const Tile t = in.tiles[tile];
    const KArgs a = args_of(in, t);
    const Thread th = thread_of(in, tile);
    const uint32_t tid = th.tid, lane = th.lane, wave = th.wave, id = th.id;
    if (tid == 0u) s_cnt = 0u; // (visible behind build_bundles' first barrier)
    const bool pending = th.pending;
    const Ray r2 = th.r;
    float bt = kNoHit;
    uint32_t bid = 0xffffffffu;
    uint32_t done = 0u, fills = 0u;
    if constexpr (WALK != 0) closest_of_planes(a, r2, pending, id, bt, bid);

    const uint32_t nb = build_bundles(r2, pending, t.brute != 0u, tid, lane, wave, s_red, s_bundle, s_lead_u, s_lead_lane);
    if constexpr (WALK != 0) {
        if (nb != 0u && a.ns != 0u) {
            const bool wave_open = __ballot(pending) != 0ull;
            walk_spheres<kTileList>(a, tid, lane, s_cand, s_cand_pos, nullptr, &s_cnt, out.longest + tile, MayMeetBundles{s_bundle, nb}, [&](uint32_t cnt) {
                record_filling(out, t, tid, s_cand, s_cand_pos, nullptr, cnt, done, fills);
                if (wave_open) closest_of_list(a, r2, pending, id, s_cand, s_cand_pos, cnt, bt, bid);
            });
        }
    }
    const size_t k = (size_t)tile * kThreads + tid;
    out.nb[k] = nb;
    if (tid < nb && tid < (uint32_t)kReflectBundles) put_bundle(out.bundle + kBundleWords * ((size_t)tile * kReflectBundles + tid), s_bundle[tid]);
    if constexpr (WALK != 0) {
        out.hit[2 * k] = __float_as_uint(bt);
        out.hit[2 * k + 1] = bid;
        if (tid == 0u) {
            out.nfill[tile] = fills;
            out.rec_n[tile] = done;
        }
    }
}

// ---- the flat evaluators: one thread per pair

// may_occlude(cone, L, sphere): cones 7 words each (as put_cone writes them) with their lights, pairs (cone, sphere).
__global__ void k_may_occlude(const uint32_t* cones, const float* lights, const float4* sph, const uint2* pairs, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = cones + kConeWords * pairs[i].x;
    rtxshadow::Cone c;
    c.ax = __uint_as_float(w[0]); c.ay = __uint_as_float(w[1]); c.az = __uint_as_float(w[2]);
    c.theta = __uint_as_float(w[3]); c.dmax = __uint_as_float(w[4]); c.slack = __uint_as_float(w[5]);
    c.all = w[6] != 0u;
    const float Lf[3] = {lights[3 * pairs[i].x], lights[3 * pairs[i].x + 1], lights[3 * pairs[i].x + 2]};
    const float4 g = sph[pairs[i].y];
    out[i] = rtxshadow::may_occlude(c, Lf, g.x, g.y, g.z, g.w) ? 1u : 0u;
}

// may_hit(bundle, sphere): bundles 10 words each (as put_bundle writes them), pairs (bundle, sphere).
__global__ void k_may_hit(const uint32_t* bundles, const float4* sph, const uint2* pairs, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = bundles + kBundleWords * pairs[i].x;
    rtxreflect::Bundle b;
    b.ox = __uint_as_float(w[0]); b.oy = __uint_as_float(w[1]); b.oz = __uint_as_float(w[2]); b.rho = __uint_as_float(w[3]);
    b.ax = __uint_as_float(w[4]); b.ay = __uint_as_float(w[5]); b.az = __uint_as_float(w[6]); b.theta = __uint_as_float(w[7]);
    b.slack = __uint_as_float(w[8]);
    b.all = w[9] != 0u;
    const float4 g = sph[pairs[i].y];
    out[i] = rtxreflect::may_hit(b, g.x, g.y, g.z, g.w) ? 1u : 0u;
}

// The exact tests on the grid (point p, sphere j), pair p + npts * j: KIND 0 segment_hits_sphere of (P, L) with toL and inv_len2
// as the shadow passes form them; KIND 1 secondary_sphere_hit of the ray (O, D), a hit being one closest_of_list would take
// (reported, and t < kNoHit).  out: a byte per pair.
template <int KIND>
__global__ void k_exact(const float* A, const float* B, uint32_t npts, const float4* sph, uint32_t ns, uint8_t* out)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (size_t)npts * ns) return;
    const uint32_t p = (uint32_t)(i % npts), j = (uint32_t)(i / npts);
    const V3 x = v3(A[3 * p], A[3 * p + 1], A[3 * p + 2]), y = v3(B[3 * p], B[3 * p + 1], B[3 * p + 2]);
    const float4 g = sph[j];
    bool hit;
    if constexpr (KIND == 0) {
        const V3 toL = sub(y, x);
        const float len2 = dot(toL, toL);
        const float inv_len2 = len2 > 0.0f ? 1.0f / len2 : 0.0f;
        hit = segment_hits_sphere(x, toL, inv_len2, g);
    } else {
        Ray r;
        r.o = x;
        r.d = y;
        r.a = dot(r.d, r.d);
        r.fourA = 4.0f * r.a;
        r.divTwoA = rcp_cr(2.0f * r.a);
        float t = 0.0f;
        hit = secondary_sphere_hit(r, g, t) && t < kNoHit;
    }
    out[i] = hit ? 1u : 0u;
}

// Device copies of the inputs and outputs of one call, freed when it returns.
struct Buffers {
    std::vector<void*> held;
    bool ok = true;
    void* up(const void* src, size_t bytes)
    {
        void* d = nullptr;
        ok = ok && hipMalloc(&d, bytes ? bytes : 4) == hipSuccess;
        if (ok) held.push_back(d);
        ok = ok && (src == nullptr ? hipMemset(d, 0, bytes ? bytes : 4) : hipMemcpy(d, src, bytes, hipMemcpyHostToDevice)) == hipSuccess;
        return d;
    }
    // nullptr stays nullptr
    template <class T>
    const T* in(const T* src, size_t count) { return src ? (const T*)up(src, count * sizeof(T)) : nullptr; }
    template <class T>
    T* out(T* dst, size_t count) { return dst ? (T*)up(nullptr, count * sizeof(T)) : nullptr; }
    bool down(void* dst, const void* d, size_t bytes) { return ok = ok && (dst == nullptr || hipMemcpy(dst, d, bytes, hipMemcpyDeviceToHost) == hipSuccess); }
    bool ran() { return ok = ok && hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess; }
    ~Buffers()
    {
        for (void* d : held) hipFree(d);
    }
};

enum Mode { kCone, kShadowWalk, kDarkSet, kBundles, kMirrorWalk };

// Everything a kernel of `mode` indexes with the caller's numbers, checked here: nothing is launched otherwise.
bool fits(Mode mode, const TileIn& in, const TileOut& out)
{
    if (!in.tiles || !in.flags || in.ntiles == 0 || in.ntiles > (1u << 16) || in.npts > (uint32_t)kThreads) return false;
    if (in.nsph > (1u << 24) || in.npl > 16u || in.nlights > (1u << 20) || out.nrec > (1u << 24)) return false;
    if ((in.nsph != 0 && (!in.sph_geom || !in.sph_od)) || (in.npl != 0 && (!in.pl_a || !in.pl_b || !in.pl_od))) return false;
    const bool shadow = mode == kCone || mode == kShadowWalk || mode == kDarkSet, mirror = mode == kBundles || mode == kMirrorWalk;
    const bool walk = mode == kShadowWalk || mode == kMirrorWalk;
    if (shadow && (!in.P || !in.lights)) return false;
    if (mode == kDarkSet && !in.N) return false;
    if (mirror && (!in.O || !in.D)) return false;
    if (mode != kCone && mode != kBundles && !in.id) return false;
    if ((mode == kCone || mode == kShadowWalk) && (!out.verdict || !out.cone)) return false;
    if ((mode == kShadowWalk || mode == kDarkSet) && !out.flag) return false;
    if (mirror && (!out.nb || !out.bundle)) return false;
    if (mode == kMirrorWalk && !out.hit) return false;
    if (mode != kCone && mode != kBundles && !out.longest) return false;
    if (walk && (!out.nfill || !out.rec_n || (out.nrec != 0 && !out.rec))) return false;
    for (uint32_t k = 0; k < in.ntiles; k++) {
        const Tile& t = in.tiles[k];
        if ((uint64_t)t.sph_off + t.ns > in.nsph || t.np > in.npl) return false;
        if (shadow && (t.nl < 1u || t.nl > (uint32_t)rtxlights::kMaxLights || (uint64_t)t.light_off + t.nl > in.nlights)) return false;
        if (walk && (uint64_t)t.rec_off + t.rec_cap > out.nrec) return false;
        if (in.id) {
            for (uint32_t p = 0; p < in.npts; p++) {
                const uint32_t id = in.id[(size_t)k * in.npts + p];
                if (!(id & 0x80000000u) && id >= t.ns) return false;
            }
        }
    }
    return true;
}

int run(Mode mode, const TileIn* hin, const TileOut* hout)
{
    if (!hin || !hout || !fits(mode, *hin, *hout)) return -2;
    const size_t nt = hin->ntiles, np = nt * hin->npts, nth = nt * kThreads;
    Buffers b;
    TileIn in = *hin;
    TileOut out = *hout;
    in.tiles = b.in(hin->tiles, nt);
    in.flags = b.in(hin->flags, np);
    in.P = b.in(hin->P, np * 3);
    in.N = b.in(hin->N, np * 3);
    in.id = b.in(hin->id, np);
    in.O = b.in(hin->O, np * 3);
    in.D = b.in(hin->D, np * 3);
    // (a tile with no sphere or plane still hands the kernels a pointer: nothing is read through it)
    in.sph_geom = (const float4*)b.up(hin->nsph ? hin->sph_geom : nullptr, (size_t)hin->nsph * 16);
    in.sph_od = (const float4*)b.up(hin->nsph ? hin->sph_od : nullptr, (size_t)hin->nsph * 16);
    in.pl_a = (const float4*)b.up(hin->npl ? hin->pl_a : nullptr, (size_t)hin->npl * 16);
    in.pl_b = (const float4*)b.up(hin->npl ? hin->pl_b : nullptr, (size_t)hin->npl * 16);
    in.pl_od = (const float4*)b.up(hin->npl ? hin->pl_od : nullptr, (size_t)hin->npl * 16);
    in.lights = b.in(hin->lights, (size_t)hin->nlights * 3);
    out.verdict = b.out(hout->verdict, nth);
    out.cone = b.out(hout->cone, nth * kConeWords);
    out.flag = b.out(hout->flag, nth);
    out.hit = b.out(hout->hit, nth * 2);
    out.nb = b.out(hout->nb, nth);
    out.bundle = b.out(hout->bundle, nt * kReflectBundles * kBundleWords);
    out.longest = b.out(hout->longest, nt);
    out.nfill = b.out(hout->nfill, nt);
    out.rec_n = b.out(hout->rec_n, nt);
    out.rec = b.out(hout->rec, (size_t)hout->nrec * kRecWords);
    if (!b.ok) return -1;
    const dim3 grid((uint32_t)nt), block(kThreads);
    switch (mode) {
    case kCone: hipLaunchKernelGGL(k_cone, grid, block, 0, 0, in, out); break;
    case kShadowWalk: hipLaunchKernelGGL(k_shadow_walk, grid, block, 0, 0, in, out); break;
    case kDarkSet: hipLaunchKernelGGL(k_dark_set, grid, block, 0, 0, in, out); break;
    case kBundles: hipLaunchKernelGGL(k_mirror<0>, grid, block, 0, 0, in, out); break;
    case kMirrorWalk: hipLaunchKernelGGL(k_mirror<1>, grid, block, 0, 0, in, out); break;
    }
    b.ran();
    b.down(hout->verdict, out.verdict, nth * 4);
    b.down(hout->cone, out.cone, nth * kConeWords * 4);
    b.down(hout->flag, out.flag, nth * 4);
    b.down(hout->hit, out.hit, nth * 8);
    b.down(hout->nb, out.nb, nth * 4);
    b.down(hout->bundle, out.bundle, nt * kReflectBundles * kBundleWords * 4);
    b.down(hout->longest, out.longest, nt * 4);
    b.down(hout->nfill, out.nfill, nt * 4);
    b.down(hout->rec_n, out.rec_n, nt * 4);
    b.down(hout->rec, out.rec, (size_t)hout->nrec * kRecWords * 4);
    return b.ok ? 0 : -1;
}

bool pairs_fit(const uint32_t* pairs, unsigned n, unsigned nitems, unsigned nsph)
{
    for (unsigned i = 0; i < n; i++) {
        if (pairs[2 * i] >= nitems || pairs[2 * i + 1] >= nsph) return false;
    }
    return n > 0 && n < (1u << 28);
}

} // namespace

static_assert(sizeof(Tile) == kTileWords * 4, "a tile is 8 words");

#define RTX_CHECK_API extern "C" __attribute__((visibility("default")))

RTX_CHECK_API int rtx_tile_cone(const TileIn* in, const TileOut* out) { return run(kCone, in, out); }
RTX_CHECK_API int rtx_tile_shadow_walk(const TileIn* in, const TileOut* out) { return run(kShadowWalk, in, out); }
RTX_CHECK_API int rtx_tile_dark_set(const TileIn* in, const TileOut* out) { return run(kDarkSet, in, out); }
RTX_CHECK_API int rtx_tile_bundles(const TileIn* in, const TileOut* out) { return run(kBundles, in, out); }
RTX_CHECK_API int rtx_tile_mirror_walk(const TileIn* in, const TileOut* out) { return run(kMirrorWalk, in, out); }

// out: n words, 1 where rtxshadow::may_occlude keeps the pair's sphere for the pair's cone (7 words) and light (3 floats).
RTX_CHECK_API int rtx_tile_may_occlude(const uint32_t* cones, const float* lights, unsigned ncones, const float* spheres, unsigned ns, const uint32_t* pairs,
                                       unsigned n, uint32_t* out)
{
    if (!cones || !lights || !spheres || !pairs || !out || !pairs_fit(pairs, n, ncones, ns)) return -2;
    Buffers b;
    const uint32_t* d_cones = (const uint32_t*)b.up(cones, (size_t)ncones * kConeWords * 4);
    const float* d_lights = (const float*)b.up(lights, (size_t)ncones * 12);
    const float4* d_sph = (const float4*)b.up(spheres, (size_t)ns * 16);
    const uint2* d_pairs = (const uint2*)b.up(pairs, (size_t)n * 8);
    uint32_t* d_out = (uint32_t*)b.up(nullptr, (size_t)n * 4);
    if (!b.ok) return -1;
    hipLaunchKernelGGL(k_may_occlude, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, 0, d_cones, d_lights, d_sph, d_pairs, (uint32_t)n, d_out);
    return b.ran() && b.down(out, d_out, (size_t)n * 4) ? 0 : -1;
}

// out: n words, 1 where rtxreflect::may_hit keeps the pair's sphere for the pair's bundle (10 words).
RTX_CHECK_API int rtx_tile_may_hit(const uint32_t* bundles, unsigned nbundles, const float* spheres, unsigned ns, const uint32_t* pairs, unsigned n, uint32_t* out)
{
    if (!bundles || !spheres || !pairs || !out || !pairs_fit(pairs, n, nbundles, ns)) return -2;
    Buffers b;
    const uint32_t* d_bundles = (const uint32_t*)b.up(bundles, (size_t)nbundles * kBundleWords * 4);
    const float4* d_sph = (const float4*)b.up(spheres, (size_t)ns * 16);
    const uint2* d_pairs = (const uint2*)b.up(pairs, (size_t)n * 8);
    uint32_t* d_out = (uint32_t*)b.up(nullptr, (size_t)n * 4);
    if (!b.ok) return -1;
    hipLaunchKernelGGL(k_may_hit, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, 0, d_bundles, d_sph, d_pairs, (uint32_t)n, d_out);
    return b.ran() && b.down(out, d_out, (size_t)n * 4) ? 0 : -1;
}

// kind 0: segment_hits_sphere of the segments (A[p], B[p]) = (P, L); kind 1: secondary_sphere_hit of the rays (A[p], B[p]) = (O, D).
// out: ns x npts bytes, out[j * npts + p] = 1 where point / ray p hits sphere j.
RTX_CHECK_API int rtx_tile_exact(int kind, const float* A, const float* B, unsigned npts, const float* spheres, unsigned ns, uint8_t* out)
{
    if (!A || !B || !spheres || !out || (kind != 0 && kind != 1) || npts == 0 || ns == 0 || (uint64_t)npts * ns >= (1ull << 28)) return -2;
    Buffers b;
    const float* d_A = (const float*)b.up(A, (size_t)npts * 12);
    const float* d_B = (const float*)b.up(B, (size_t)npts * 12);
    const float4* d_sph = (const float4*)b.up(spheres, (size_t)ns * 16);
    uint8_t* d_out = (uint8_t*)b.up(nullptr, (size_t)npts * ns);
    if (!b.ok) return -1;
    const dim3 grid((uint32_t)(((size_t)npts * ns + kThreads - 1) / kThreads)), block(kThreads);
    if (kind == 0) {
        hipLaunchKernelGGL(k_exact<0>, grid, block, 0, 0, d_A, d_B, (uint32_t)npts, d_sph, (uint32_t)ns, d_out);
    } else {
        hipLaunchKernelGGL(k_exact<1>, grid, block, 0, 0, d_A, d_B, (uint32_t)npts, d_sph, (uint32_t)ns, d_out);
    }
    return b.ran() && b.down(out, d_out, (size_t)npts * ns) ? 0 : -1;
}
