// rtx_kernels.hip -- gfx950 kernels of the ray-trace hot path.
//
// One thread per pixel per pass (as the reference, RayTracingManager.cu:120-125).  A 256-thread workgroup owns a macro tile
// of NSUB sub-tiles, each 2^lw x 2^(8-lw) pixels, and handles one sub-tile per pass.  Once per workgroup: the spheres it has
// to consider -- the whole scene, or the list of its coarse cell (rtx_bin_cells; lists may outlive the frame, rtx_plan.hpp) --
// are walked 512 at a time (two coalesced float4 loads per thread, the next step prefetched), the ray-independent terms
// otc = o - c and cc = Dot(otc,otc) - r*r are hoisted (Sphere.cu:34-37), spheres whose inflated bound cannot touch the macro
// tile's pyramid are culled (CULL), and survivors are appended to a candidate list in LDS; the per-column and per-row terms
// of ray generation, the decimal-digit table, the glyph ramp and the planes the tile can see are staged in LDS as well.
// Then, per sub-tile, every thread runs the reference's exact ray/sphere test over the list (wave-uniform index, LDS broadcast
// reads; REFINE: over the part of it that can touch the wave's own 64 pixels) and the plane tests from the LDS table.  The
// winner alone is shaded and encoded (the reference re-derives normal/colour on every improving hit, RayTracing.cu:123-135,
// but only the last survives).
//
// Closest hit = lexicographic minimum of (t, creation order): the same object the reference's in-order scan with strict '<'
// keeps (RayTracing.cu:123).  Spheres are known by their position in the arrays the kernel reads (KArgs::sph_geom: the
// direction-sorted copies when there are some); the creation order is looked up only in an exact tie (comes_first).
#include <stdio.h>

#include <type_traits>

#include "rtx_cull.hpp"
#include "rtx_device.hpp"
#include "rtx_far.hpp"
#include "rtx_kernels.h"
#include "rtx_records.hpp"
#include "rtx_reflect.hpp"
#include "rtx_shadow.hpp"
#include "rtx_workgroup.hpp"

// The experiment build's hooks (ABL, STAMP, RTX_X_*): empty / constant false in the product build.
#define RTX_X_SECTION_DEVICE
#include "rtx_experiment.inc"
#undef RTX_X_SECTION_DEVICE
#define RTX_X_SECTION_HOST
#include "rtx_experiment.inc"
#undef RTX_X_SECTION_HOST

namespace rtx {

// (rtx_workgroup.hpp: lds_barrier, kThreads, kChunk, kNoHit)
constexpr int kListCapBrute = 1024;  // candidate records per flush (brute: every sphere is a candidate)
constexpr int kListCapCull = 704;    // culling kernels: room for one more 512-sphere step while <= 192 are listed; 8 workgroups per CU
constexpr int kListCapRefine = 640;  // REFINE: ... while <= 128 are listed

// RayTracing.h:97-115 (68 glyphs).
__constant__ __attribute__((aligned(4))) const char kRamp[68] = {
    ' ', '.', '`', '^', '"', ',', ':', ';', 'I', 'l', '!', 'i', '>', '<', '~', '+', '_',
    '-', '?', '*', ']', '[', '}', '{', '1', ')', '(', '|', '/', 't', 'f', 'j', 'r', 'x',
    'n', 'u', 'v', 'c', 'z', 'm', 'w', 'X', 'Y', 'U', 'J', 'C', 'L', 'q', 'p', 'd', 'b',
    'k', 'h', 'a', 'o', '#', '%', 'Z', 'O', '8', 'B', '$', '0', 'Q', 'M', '&', 'W', '@'
};

struct Best {
    float t;
    uint32_t k; // the sphere's position in the arrays staging reads (= its index without sorted copies), or 0xffffffff
};

// Does the sphere at position p come before the one at position q in creation order?  (The reference keeps the first of two
// objects at the same distance, RayTracing.cu:123; q = 0xffffffff: no sphere yet.)  Rare path: the translation table's address
// is parked in LDS (rare[kRareSortedIdx]; 0 = positions are sphere indices), two loads when the arrays are sorted.
constexpr int kRareSortedIdx = 4;
__device__ __forceinline__ bool comes_first(const unsigned long long* rare, uint32_t p, uint32_t q)
{
    asm volatile("" ::: "memory"); // (keeps the read below in this branch instead of hoisting it out of the candidate loop)
    const uint32_t* sorted_idx = reinterpret_cast<const uint32_t*>((uintptr_t)rare[kRareSortedIdx]);
    if (q == 0xffffffffu || sorted_idx == nullptr) {
        return p < q;
    }
    return sorted_idx[p] < sorted_idx[q];
}

template <int MODE>
__device__ __forceinline__ Fields pixel_fields(const KArgs& a, const uint8_t* s_ramp, V3 normal, V3 colour, float shadingValue)
{
    constexpr bool kRgb = (MODE == RTX_K_RGB_ASCII || MODE == RTX_K_RGB_PIXEL || MODE == RTX_K_RGB_NORMALS);
    Fields f;
    if (kRgb) {
        if (MODE == RTX_K_RGB_NORMALS) {
            f.c0 = u8_sat(normal.x * 255.0f);
            f.c1 = u8_sat(normal.y * 255.0f);
            f.c2 = u8_sat(normal.z * 255.0f);
        } else {
            f.c0 = u8_clamped(colour.x);
            f.c1 = u8_clamped(colour.y);
            f.c2 = u8_clamped(colour.z);
        }
        f.glyph = (MODE == RTX_K_RGB_ASCII) ? (uint32_t)s_ramp[ramp_index(shadingValue)] : (uint32_t)' ';
    } else {
        f.c0 = ansi256_from_rgb(u8_clamped(colour.x), u8_clamped(colour.y), u8_clamped(colour.z), a.grey);
        f.c1 = f.c2 = 0u;
        f.glyph = (MODE == RTX_K_BIT_ASCII) ? (uint32_t)s_ramp[ramp_index(shadingValue)] : (uint32_t)' ';
    }
    return f;
}

// OUT: what a pixel's result is stored as -- a kernel per form, so that the frame loop's kernel carries no
// trace of the other two.
// kOutHit: the first launch of the light / shadow path -- the closest hit alone (t, and which object), 8 bytes per pixel, for
// rtx_shadow_shade (rtx_shadow_kernels.inc); no shading, nothing encoded.
enum { kOutRecords = 0, kOutCompact = 1, kOutValues = 2, kOutHit = 3 };

template <int MODE, int OUT>
__device__ __forceinline__ void encode_and_store(const KArgs& a, const Camera& cam, const uint32_t* s_digits, const uint8_t* s_ramp, bool in_frame, bool is_newline_col,
                                                 uint32_t row, uint32_t col, float distance, V3 normal, V3 colour, float shadingValue)
{
    constexpr bool kRgb = (MODE == RTX_K_RGB_ASCII || MODE == RTX_K_RGB_PIXEL || MODE == RTX_K_RGB_NORMALS);
    constexpr uint32_t S = kRgb ? 20u : 12u;
    if (!in_frame) {
        return;
    }
    const bool visible = distance <= cam.far; // RayTracing.cu:207,288,371,508,646
    if (OUT == kOutValues) {
        // RTX_RENDER_VALUES: the floats behind the record (RayTraceReturnData, RayTracing.h:17-23), for parity checks
        float4* o = reinterpret_cast<float4*>(a.out) + ((size_t)(row - a.out_row_base) * a.W + col) * 2u;
        if (is_newline_col) {
            o[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            o[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            o[0] = make_float4(distance, shadingValue, normal.x, normal.y);
            o[1] = make_float4(normal.z, colour.x, colour.y, colour.z);
        }
        return;
    }
    if (OUT == kOutCompact) {
        uint32_t word = kCompactNewline;
        if (!is_newline_col) {
            word = kCompactMiss;
            if (visible) {
                const Fields f = pixel_fields<MODE>(a, s_ramp, normal, colour, shadingValue);
                word = f.c0 | (f.c1 << 8) | (f.c2 << 16) | (f.glyph << 24);
            }
        }
        reinterpret_cast<uint32_t*>(a.out)[(size_t)(row - a.out_row_base) * a.W + col] = word;
        return;
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.out + ((size_t)(row - a.out_row_base) * a.W + col) * S);
    if (is_newline_col) {
        // column W-1 stays NUL (RayTracing.cu:187 never writes it; the reference memsets it)
#pragma unroll
        for (uint32_t i = 0; i < S / 4u; i++) {
            dst[i] = 0u;
        }
        return;
    }
    uint32_t w[5];
    Fields f = {0u, 0u, 0u, 0u};
    if (visible) {
        f = pixel_fields<MODE>(a, s_ramp, normal, colour, shadingValue);
    }
    record_words<MODE>(visible, f, s_digits, w);
#pragma unroll
    for (uint32_t i = 0; i < S / 4u; i++) {
        dst[i] = w[i];
    }
}

// Exact tests of one ray against the candidate list (index is wave-uniform: LDS broadcast reads).
// ray.divTwoA was filled before the loop, once per ray (half_recip, or the REFINE kernels' rcp_cr).
__device__ __forceinline__ void test_candidate(Ray& ray, const float4 sr, const uint32_t* s_idx, const unsigned long long* rare, uint32_t i, Best& best, uint32_t& slow)
{
    float s;
    const bool rejected = sphere_reject(ray, sr.x, sr.y, sr.z, sr.w, s);
    RTX_X_CANDIDATE_BEGIN();
    if (!rejected) {
        float t;
        if (sphere_hit(ray, s, sr.w, t)) {
            const uint32_t ki = s_idx[i];
            if (t < best.t || (t == best.t && comes_first(rare, ki, best.k))) {
                best.t = t;
                best.k = ki;
                RTX_X_CANDIDATE_UPDATED();
            }
        }
    }
    RTX_X_CANDIDATE_END(rejected, slow);
}
__device__ __forceinline__ void scan_candidates(Ray& ray, const float4* s_rec, const uint32_t* s_idx, const unsigned long long* rare, uint32_t total, Best& best,
                                                uint32_t& slow)
{
    for (uint32_t i = 0; i < total; i++) {
        test_candidate(ray, s_rec[i], s_idx, rare, i, best, slow);
    }
}

// Work estimate of one wave's pass over one sub-tile, in VALU instructions (tools/ablate_pmc_gpu.sh: about 100 for
// ray generation, planes and a miss record; 3 per candidate rejected; 330 more when anything is hit: the hit tests'
// slow path, the winner's normal, shading and the record).  Only the order of the sums matters.
constexpr uint32_t kCostPass = 100u, kCostCandidate = 3u, kCostShaded = 330u;

constexpr int kMaxMacro = 128;    // macro tile is at most 128 x 128 pixels
constexpr int kMaxMacroRefine = 64; // ... 64 x 64 for the REFINE kernels
constexpr int kPlaneTable = 16;   // planes hoisted into LDS; further planes take the direct path
constexpr uint32_t kPlaneRow = 5; // float4s per plane in that table (rtx_trace_body.inc: s_plane)

constexpr uint32_t kStageFull = 0xffffffffu; // stage_chunk: the step's survivors would not fit the list (nothing was written)

// One staging step: items [base, base + 512) of `ns` items, two per thread.  g0/g1 (sphere indices k0/k1)
// are this thread's geometry records, already loaded: the caller prefetches the next step's first.  Hoists the
// ray-independent terms, culls, and appends survivors to the LDS list in index order (wave ballots,
// per-wave counts through LDS, one barrier).  Returns the new list length (uniform), or kStageFull when the step's
// survivors would take the list past `cap` entries (then nothing is written).
// (Keeping the geometry and colour records of the first list entries in LDS, so that a pass takes its winner's records
// from there instead of a round trip to memory, was measured and dropped: no gain, profiles/r02_c_single_launch_experiments.md.)
template <bool CULL>
__device__ __forceinline__ uint32_t stage_chunk(const Camera& cam, const TileFrustum& fr, uint32_t ns, uint32_t base, float4 g0, float4 g1,
                                                uint32_t k0, uint32_t k1, float4* s_rec, uint32_t* s_idx, uint32_t (*s_wcnt)[8],
                                                uint32_t parity, uint32_t total, bool drop_all, uint32_t cap, float* s_margin = nullptr)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    bool keep[2];
    float4 rec[2];
    float mg[2] = {0.0f, 0.0f};
    const float4 g[2] = {g0, g1};

    // the second half of the step is empty when at most 256 items are left (short cell lists, the tail of a scene):
    // skip its arithmetic (uniform branch)
    const bool second_half_empty = base + (uint32_t)kThreads >= ns;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if (h == 1 && second_half_empty) {
            keep[1] = false;
            rec[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            break;
        }
        const uint32_t k = base + (uint32_t)h * kThreads + tid; // item number; valid while below ns (the item count)
        // objectToCam = origin - spherePos; c = Dot(otc,otc) - r*r   (Sphere.cu:34-37)
        const float ox = cam.ox - g[h].x, oy = cam.oy - g[h].y, oz = cam.oz - g[h].z;
        const float oo = ox * ox + oy * oy + oz * oz;
        const float cc = oo - (g[h].w * g[h].w);
        rec[h] = make_float4(ox, oy, oz, cc);
        keep[h] = (k < ns) && !drop_all;
        if (CULL) {
            // cc <= 0: the camera is inside or on the sphere; keep (the exact test decides)
            const bool culled = tile_culls(fr, ox, oy, oz, oo, g[h].w, mg[h]);
            keep[h] = keep[h] && !(cc > 0.0f && culled);
            if (!(cc > 0.0f)) {
                mg[h] = __builtin_inff(); // camera inside or on the sphere: never culled, by any pyramid
            }
        }
    }
    const unsigned long long m0 = __ballot(keep[0]), m1 = __ballot(keep[1]);
    if (lane == 0) {
        s_wcnt[parity][wave] = (uint32_t)__popcll(m0);
        s_wcnt[parity][4 + wave] = (uint32_t)__popcll(m1);
    }
    // LDS-only barrier: the caller's prefetched global loads stay in flight across it.  It also orders
    // the previous scan's list reads before the writes below.
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < 8u; w++) {
        const uint32_t c = s_wcnt[parity][w];
        sum += c;
        if (w < wave) before += c; // first halves of earlier waves (wave <= 3)
    }
    // a step whose survivors do not fit the list is not written at all (uniform: every thread sees the same counts)
    const uint32_t grown = __builtin_amdgcn_readfirstlane(total + sum);
    if (grown > cap) {
        return kStageFull;
    }
    // index order: [first-half survivors of waves 0..3][second-half survivors of waves 0..3]
    uint32_t first_total = 0, before1 = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4u; w++) {
        first_total += s_wcnt[parity][w];
        if (w < wave) before1 += s_wcnt[parity][4 + w];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (keep[0]) {
        const uint32_t pos = total + before + (uint32_t)__popcll(m0 & below);
        s_rec[pos] = rec[0];
        s_idx[pos] = k0;
        if (s_margin) s_margin[pos] = mg[0];
    }
    if (keep[1]) {
        const uint32_t pos = total + first_total + before1 + (uint32_t)__popcll(m1 & below);
        s_rec[pos] = rec[1];
        s_idx[pos] = k1;
        if (s_margin) s_margin[pos] = mg[1];
    }
    return grown;
}

// (rtx_workgroup.hpp: Items, scene_items, load_item -- the spheres a workgroup stages)

constexpr int kRefineSub = 4;      // REFINE: at most this many sub-tiles (lanes 5 .. 5 + 16 per sub-tile build the pyramids)
constexpr int kWaveListCap = 128;  // REFINE: candidates a wave keeps for its own 64 pixels; more -> it scans the whole list

// REFINE (dense scenes, long candidate lists): before a wave scans the workgroup's list for its 64 pixels it
// tests the list, one entry per lane, against the pyramid of just those pixels -- same conservative test and
// margin as for the macro tile -- and scans the survivors only.
#ifndef RTX_WAVES_PER_EU
#define RTX_WAVES_PER_EU 7 // 72 VGPRs: 7 workgroups per CU instead of 6 (20.4 -> 19.6 us per frame; 8 needs spills and gains nothing)
#endif
// Where a workgroup stands: in a plain launch the grid is the frame's tile grid; in a batched one (rtx_trace_batch) it is 1-D,
// workgroup b on tile position b / n of frame b % n.  Computed where they are used (at the head and at the very end of the
// kernel), from the block index, rather than carried in scalar registers across the pass loop.
template <bool BATCH>
struct Where {
    static __device__ __forceinline__ uint32_t pos(const KArgs& a) { return BATCH ? blockIdx.x / a.batch_n : blockIdx.y * gridDim.x + blockIdx.x; }
    static __device__ __forceinline__ uint32_t grid_x(const KArgs& a) { return BATCH ? a.batch_gx : gridDim.x; }
    static __device__ __forceinline__ uint32_t n_tiles(const KArgs& a) { return BATCH ? a.batch_gx * a.batch_gy : gridDim.x * gridDim.y; }
    static __device__ __forceinline__ bool first_block() { return BATCH ? blockIdx.x == 0u : (blockIdx.x == 0u && blockIdx.y == 0u); }
    // one frame of a batch leaves the work estimates (the tiles' costs differ little from frame to frame of a round)
    static __device__ __forceinline__ bool leaves_cost(const KArgs& a) { return BATCH ? blockIdx.x % a.batch_n == 0u : true; }
};

// The body of the trace kernels lives in rtx_trace_body.inc, included into the two entry points below.
template <int MODE, bool CULL, int OUT, bool REFINE>
__global__ __launch_bounds__(kThreads, RTX_WAVES_PER_EU) void rtx_trace(const KArgs a)
{
    constexpr bool BATCH = false;
#include "rtx_trace_body.inc"
}

// The same rows of a.batch_n frames in one launch (KBatch, rtx_kernels.h): a 1-D grid of batch_n x tiles workgroups, workgroup b
// on tile position b / batch_n of frame b % batch_n.  The frame's camera, edge basis and output buffer replace the launch's.
template <int MODE, int OUT>
__global__ __launch_bounds__(kThreads, RTX_WAVES_PER_EU) void rtx_trace_batch(const KArgs a0, const KBatch kb)
{
    const uint32_t frame = blockIdx.x % a0.batch_n;
    KArgs a = a0;
    const KFrame& f = kb.f[frame];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        a.m[i] = f.m[i];
    }
    a.ox = f.ox;
    a.oy = f.oy;
    a.oz = f.oz;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        a.edge_up_p[i] = f.edge_up_p[i];
        a.edge_up_q[i] = f.edge_up_q[i];
        a.edge_right_p[i] = f.edge_right_p[i];
        a.edge_right_q[i] = f.edge_right_q[i];
        a.edge_fwd[i] = f.edge_fwd[i];
    }
    a.edge_pp = f.edge_pp;
    a.edge_qrqr = f.edge_qrqr;
    a.edge_qcqc = f.edge_qcqc;
    a.out = f.out;
    constexpr bool BATCH = true, CULL = true, REFINE = false;
#include "rtx_trace_body.inc"
}

// Level 1 of the two-level culling used for large scenes: rtx_bin_cells, with the rule it is launched by.
#include "rtx_bin_cells.inc"

// Zero-fills [begin, end) of the frame (bytes, 4-aligned): the 8-bit modes' unused tail.
__global__ __launch_bounds__(kThreads) void rtx_zero_fill(uint32_t* p, size_t n_words)
{
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n_words; i += (size_t)gridDim.x * kThreads) {
        p[i] = 0u;
    }
}

// The passes that write a dispatch order, rtx_order_tiles and rtx_balance_tiles, with the rules they are launched by.
#include "rtx_order_kernels.inc"

// rtx_expand: compact pixel words -> records, for up to kMaxExpandSeg segments (a segment = a run of pixels that
// is contiguous in both buffers: one rank's rows of one frame).  Pure streaming: 4 bytes read, S written per pixel.
// A workgroup takes kExpandPixels consecutive pixels of one segment, 256 at a time; each wave transposes the
// records of its 64 pixels through its own piece of LDS (pixel p at dword p*S/4, odd stride: conflict-free), so
// that its 64*S bytes leave as whole 16-byte stores in address order -- wave-local, no workgroup barrier.
template <int MODE>
__global__ __launch_bounds__(kThreads) void rtx_expand_words(const ExpandArgs e)
{
    constexpr bool kRgb = (MODE == RTX_K_RGB_ASCII || MODE == RTX_K_RGB_PIXEL || MODE == RTX_K_RGB_NORMALS);
    constexpr uint32_t SW = kRgb ? 5u : 3u; // dwords per record
    __shared__ uint32_t s_digits[256];
    __shared__ __attribute__((aligned(16))) uint32_t s_rec[kThreads * SW];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    s_digits[tid] = digits_word(tid);
    uint32_t k = 0;
    while (k + 1u < e.nseg && blockIdx.x >= e.first_block[k + 1u]) {
        k++;
    }
    const uint32_t npix = e.npix[k];
    const uint32_t* src = e.src + e.src_px[k];
    uint32_t* dst_seg = reinterpret_cast<uint32_t*>(e.dst) + e.dst_px[k] * SW;
    const uint32_t base = (blockIdx.x - e.first_block[k]) * (uint32_t)kExpandPixels;
    uint32_t* s_wave = s_rec + wave * 64u * SW;
    __syncthreads();
#pragma unroll 1
    for (uint32_t c = 0; c < (uint32_t)kExpandPixels; c += (uint32_t)kThreads) {
        const uint32_t w0 = base + c + wave * 64u; // first pixel of this wave's 64
        if (w0 >= npix) {
            break;
        }
        const uint32_t p = w0 + lane;
        const bool valid = p < npix;
        const uint32_t word = valid ? src[p] : kCompactNewline;
        uint32_t w[SW];
        if (word == kCompactNewline) {
#pragma unroll
            for (uint32_t i = 0; i < SW; i++) {
                w[i] = 0u;
            }
        } else {
            Fields f;
            f.c0 = word & 255u;
            f.c1 = (word >> 8) & 255u;
            f.c2 = (word >> 16) & 255u;
            f.glyph = word >> 24;
            record_words<MODE>(word != kCompactMiss, f, s_digits, w);
        }
        uint32_t* dst = dst_seg + (size_t)w0 * SW;
        if (e.aligned16 && w0 + 64u <= npix) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the previous round's reads of s_wave are done
#pragma unroll
            for (uint32_t i = 0; i < SW; i++) {
                s_wave[lane * SW + i] = w[i];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // wave-local: LDS is in order within a wave
            const uint4* s4 = reinterpret_cast<const uint4*>(s_wave);
            uint4* d4 = reinterpret_cast<uint4*>(dst);
            constexpr uint32_t n4 = 16u * SW; // 16-byte pieces of the wave's 64 records: 80 or 48
            if (lane < n4) {
                d4[lane] = s4[lane];
            }
            if (64u + lane < n4) {
                d4[64u + lane] = s4[64u + lane];
            }
        } else if (valid) {
#pragma unroll
            for (uint32_t i = 0; i < SW; i++) {
                dst[(size_t)lane * SW + i] = w[i];
            }
        }
    }
}

#include "rtx_tile_pass.inc"
#include "rtx_reflect_kernels.inc"
#include "rtx_reflect_chain_kernels.inc"
#include "rtx_grid_reflect_kernels.inc"
#include "rtx_shadow_kernels.inc"
#include "rtx_lights_kernels.inc"
#include "rtx_lights_chain_kernels.inc"
#include "rtx_chain_shadow_kernels.inc"
#include "rtx_grid_shadow_kernels.inc"
#include "rtx_resolve_kernels.inc"
#include "rtx_query_kernels.inc"

} // namespace rtx

extern "C" int rtx_k_launch_expand(const ExpandArgs* e, int mode, unsigned blocks, void* stream_v)
{
    using namespace rtx;
    hipStream_t stream = (hipStream_t)stream_v;
    switch (mode) {
    case RTX_K_BIT_ASCII: hipLaunchKernelGGL((rtx_expand_words<RTX_K_BIT_ASCII>), dim3(blocks), dim3(kThreads), 0, stream, *e); break;
    case RTX_K_BIT_PIXEL: hipLaunchKernelGGL((rtx_expand_words<RTX_K_BIT_PIXEL>), dim3(blocks), dim3(kThreads), 0, stream, *e); break;
    case RTX_K_RGB_ASCII: hipLaunchKernelGGL((rtx_expand_words<RTX_K_RGB_ASCII>), dim3(blocks), dim3(kThreads), 0, stream, *e); break;
    case RTX_K_RGB_PIXEL: hipLaunchKernelGGL((rtx_expand_words<RTX_K_RGB_PIXEL>), dim3(blocks), dim3(kThreads), 0, stream, *e); break;
    case RTX_K_RGB_NORMALS: hipLaunchKernelGGL((rtx_expand_words<RTX_K_RGB_NORMALS>), dim3(blocks), dim3(kThreads), 0, stream, *e); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

extern "C" const char* rtx_k_launch_trace(const KArgs* a, int mode, int cull, void* stream_v, int* hip_error)
{
    using namespace rtx;
    hipStream_t stream = (hipStream_t)stream_v;
    const uint32_t lw = a->tile_log2w;
    const uint32_t tw = 1u << lw, th = (uint32_t)kThreads >> lw;
    const uint32_t nx = 1u << a->sub_log2nx, ny = a->nsub >> a->sub_log2nx;
    const uint32_t mw = tw * nx, mh = th * ny;
    *hip_error = 0;
    if (a->nsub == 0 || nx * ny != a->nsub || mw > (uint32_t)kMaxMacro || mh > (uint32_t)kMaxMacro || mw + mh > (uint32_t)kThreads) {
        return nullptr;
    }
    if (cull && a->refine && (mw > (uint32_t)kMaxMacroRefine || mh > (uint32_t)kMaxMacroRefine)) {
        return nullptr; // (rtx_render_rows does not ask for this)
    }
    const uint32_t rows = a->row_end - a->row0;
    dim3 grid((a->W + mw - 1u) / mw, (rows + mh - 1u) / mh, 1), block(kThreads, 1, 1);
    const char* name = nullptr;
    const unsigned lds_pad = rtx_x_lds_pad(); // 0 in the product build
    if (a->compact == 3u) {
        // the closest hits alone (the light / shadow path): one kernel per (CULL, REFINE), the mode does not enter
        if (mode < RTX_K_BIT_ASCII || mode > RTX_K_RGB_PIXEL) return nullptr;
        if (cull && a->refine) {
            hipLaunchKernelGGL((rtx_trace<RTX_K_RGB_PIXEL, true, kOutHit, true>), grid, block, lds_pad, stream, *a);
            name = "rtx_trace<hits,true,refine>";
        } else if (cull) {
            hipLaunchKernelGGL((rtx_trace<RTX_K_RGB_PIXEL, true, kOutHit, false>), grid, block, lds_pad, stream, *a);
            name = "rtx_trace<hits,true>";
        } else {
            hipLaunchKernelGGL((rtx_trace<RTX_K_RGB_PIXEL, false, kOutHit, false>), grid, block, lds_pad, stream, *a);
            name = "rtx_trace<hits,false>";
        }
        *hip_error = (int)hipGetLastError();
        return name;
    }
#define RTX_LAUNCH(M, C, O, SUFFIX)                                                          \
    do {                                                                                     \
        if (C && a->refine) {                                                                \
            hipLaunchKernelGGL((rtx_trace<M, C, O, C>), grid, block, lds_pad, stream, *a);   \
            name = "rtx_trace<" #M "," #C SUFFIX ",refine>";                                 \
        } else {                                                                             \
            hipLaunchKernelGGL((rtx_trace<M, C, O, false>), grid, block, lds_pad, stream, *a); \
            name = "rtx_trace<" #M "," #C SUFFIX ">";                                        \
        }                                                                                    \
    } while (0)
#define RTX_LAUNCH_OUT(M, C)                                   \
    do {                                                       \
        if (a->compact == 0u) {                                \
            RTX_LAUNCH(M, C, kOutRecords, "");                 \
        } else if (a->compact == 1u) {                         \
            RTX_LAUNCH(M, C, kOutCompact, ",compact");         \
        } else {                                               \
            RTX_LAUNCH(M, C, kOutValues, ",values");           \
        }                                                      \
    } while (0)
#define RTX_LAUNCH_MODE(M)            \
    do {                              \
        if (cull) {                   \
            RTX_LAUNCH_OUT(M, true);  \
        } else {                      \
            RTX_LAUNCH_OUT(M, false); \
        }                             \
    } while (0)
    switch (mode) {
    case RTX_K_BIT_ASCII: RTX_LAUNCH_MODE(RTX_K_BIT_ASCII); break;
    case RTX_K_BIT_PIXEL: RTX_LAUNCH_MODE(RTX_K_BIT_PIXEL); break;
    case RTX_K_RGB_ASCII: RTX_LAUNCH_MODE(RTX_K_RGB_ASCII); break;
    case RTX_K_RGB_PIXEL: RTX_LAUNCH_MODE(RTX_K_RGB_PIXEL); break;
    case RTX_K_RGB_NORMALS: RTX_LAUNCH_MODE(RTX_K_RGB_NORMALS); break;
    case RTX_K_SDL:
        // RayTrace_SDL stores nothing, whatever the output form
        if (cull) {
            RTX_LAUNCH(RTX_K_SDL, true, kOutRecords, "");
        } else {
            RTX_LAUNCH(RTX_K_SDL, false, kOutRecords, "");
        }
        break;
    default: return nullptr;
    }
#undef RTX_LAUNCH_MODE
#undef RTX_LAUNCH_OUT
#undef RTX_LAUNCH
    *hip_error = (int)hipGetLastError();
    return name;
}

extern "C" const char* rtx_k_launch_trace_batch(const KArgs* a, const KBatch* kb, int mode, void* stream_v, int* hip_error)
{
    using namespace rtx;
    hipStream_t stream = (hipStream_t)stream_v;
    const uint32_t lw = a->tile_log2w;
    const uint32_t tw = 1u << lw, th = (uint32_t)kThreads >> lw;
    const uint32_t nx = 1u << a->sub_log2nx, ny = a->nsub >> a->sub_log2nx;
    const uint32_t mw = tw * nx, mh = th * ny;
    *hip_error = 0;
    if (a->nsub == 0 || nx * ny != a->nsub || mw > (uint32_t)kMaxMacro || mh > (uint32_t)kMaxMacro || mw + mh > (uint32_t)kThreads || a->refine ||
        a->batch_n == 0 || a->batch_n > (uint32_t)kMaxBatch || a->compact > 1u) {
        return nullptr;
    }
    const uint32_t rows = a->row_end - a->row0;
    const uint64_t gx = (a->W + mw - 1u) / mw, gy = (rows + mh - 1u) / mh, blocks = gx * gy * a->batch_n;
    if (gx != a->batch_gx || gy != a->batch_gy || blocks == 0 || blocks >= (1ull << 31)) {
        return nullptr;
    }
    const dim3 grid((uint32_t)blocks, 1, 1), block(kThreads, 1, 1);
    const char* name = nullptr;
    const unsigned lds_pad = rtx_x_lds_pad(); // 0 in the product build
#define RTX_LAUNCH_BATCH(M)                                                                               \
    do {                                                                                                  \
        if (a->compact == 0u) {                                                                           \
            hipLaunchKernelGGL((rtx_trace_batch<M, kOutRecords>), grid, block, lds_pad, stream, *a, *kb); \
            name = "rtx_trace_batch<" #M ">";                                                             \
        } else {                                                                                          \
            hipLaunchKernelGGL((rtx_trace_batch<M, kOutCompact>), grid, block, lds_pad, stream, *a, *kb); \
            name = "rtx_trace_batch<" #M ",compact>";                                                     \
        }                                                                                                 \
    } while (0)
    switch (mode) {
    case RTX_K_BIT_ASCII: RTX_LAUNCH_BATCH(RTX_K_BIT_ASCII); break;
    case RTX_K_BIT_PIXEL: RTX_LAUNCH_BATCH(RTX_K_BIT_PIXEL); break;
    case RTX_K_RGB_ASCII: RTX_LAUNCH_BATCH(RTX_K_RGB_ASCII); break;
    case RTX_K_RGB_PIXEL: RTX_LAUNCH_BATCH(RTX_K_RGB_PIXEL); break;
    case RTX_K_RGB_NORMALS: RTX_LAUNCH_BATCH(RTX_K_RGB_NORMALS); break;
    default: return nullptr;
    }
#undef RTX_LAUNCH_BATCH
    *hip_error = (int)hipGetLastError();
    return name;
}

// The shade launches of the tile passes (rtx_tile_pass.inc): one workgroup per 16 x 16 tile of the launch's rows, a kernel family
// instantiated over the four character modes and the three output forms (a->compact 0 / 1 / 2).  launch(MODE, OUT, grid, block)
// -- two std::integral_constants and the grid -- launches the family's instantiation.  Returns the kernel's name as
// "family<RTX_K_mode>", "family<RTX_K_mode,compact>" or "family<RTX_K_mode,values>", or nullptr when the launch is refused.
struct ShadeNames {
    char s[4][3][64];
    explicit ShadeNames(const char* family)
    {
        static const char* const kMode[4] = {"RTX_K_BIT_ASCII", "RTX_K_BIT_PIXEL", "RTX_K_RGB_ASCII", "RTX_K_RGB_PIXEL"};
        static const char* const kSuffix[3] = {"", ",compact", ",values"};
        for (int m = 0; m < 4; m++) {
            for (int o = 0; o < 3; o++) snprintf(s[m][o], sizeof s[m][o], "%s<%s%s>", family, kMode[m], kSuffix[o]);
        }
    }
};

// The grid of a tile pass over the launch's rows; false: nothing to launch.
static bool tile_grid(const KArgs* a, dim3& grid)
{
    const uint32_t rows = a->row_end - a->row0;
    if (a->W == 0u || rows == 0u) return false;
    grid = dim3((a->W + rtx::kTile - 1u) / rtx::kTile, (rows + rtx::kTile - 1u) / rtx::kTile, 1);
    return true;
}

template <class Launch>
static const char* launch_shade(const KArgs* a, int mode, const ShadeNames& names, int* hip_error, Launch launch)
{
    using namespace rtx;
    static_assert(RTX_K_BIT_ASCII == 0 && RTX_K_RGB_PIXEL == 3 && kOutRecords == 0 && kOutCompact == 1 && kOutValues == 2, "names are indexed by mode and form");
    *hip_error = 0;
    dim3 grid;
    if (!tile_grid(a, grid) || a->compact > 2u || mode < RTX_K_BIT_ASCII || mode > RTX_K_RGB_PIXEL) return nullptr;
    const dim3 block(kThreads, 1, 1);
    const auto with_out = [&](auto m) {
        switch (a->compact) {
        case 0u: launch(m, std::integral_constant<int, kOutRecords>{}, grid, block); break;
        case 1u: launch(m, std::integral_constant<int, kOutCompact>{}, grid, block); break;
        default: launch(m, std::integral_constant<int, kOutValues>{}, grid, block); break;
        }
    };
    switch (mode) {
    case RTX_K_BIT_ASCII: with_out(std::integral_constant<int, RTX_K_BIT_ASCII>{}); break;
    case RTX_K_BIT_PIXEL: with_out(std::integral_constant<int, RTX_K_BIT_PIXEL>{}); break;
    case RTX_K_RGB_ASCII: with_out(std::integral_constant<int, RTX_K_RGB_ASCII>{}); break;
    default: with_out(std::integral_constant<int, RTX_K_RGB_PIXEL>{}); break;
    }
    *hip_error = (int)hipGetLastError();
    return names.s[mode][a->compact];
}

// What a pass or a shade family takes of TileArgs, and so what must be there for its launch: the table of the refusals.
enum : unsigned {
    kTakesShadow = 1u << 0,  // t->shadow
    kTakesLights = 1u << 1,  // t->lights, a set of 1 .. kMaxLights
    kTakesReflect = 1u << 2, // t->reflect
    kTakesChain = 1u << 3,   // t->chain, its depth in range and its stride the launch's pixels
    kTakesDeep = 1u << 4,    // t->deep with its words
    kTakesDark0 = 1u << 5,   // t->dark0
    kTakesGrid = 1u << 6,    // t->grid: a usable grid over a scene with spheres, room for level 0's words and the fallback count;
                             // reflect, chain and deep by value (they are read, and then checked, only with GridShadowArgs::deep)
    kTakesGridReflect = 1u << 7, // t->grid_reflect: a usable grid over a scene with spheres, the position map and the fallback count
};
static const unsigned kPassTakes[rtxplan::kShadePasses] = {
    0u,                                                        // kPassNone
    kTakesReflect,                                             // rtx_reflect_hit
    kTakesReflect | kTakesChain,                               // rtx_reflect_chain
    kTakesLights | kTakesReflect | kTakesChain | kTakesDeep,   // rtx_chain_shadow
    kTakesLights | kTakesGrid,                                 // rtx_grid_shadow
    kTakesReflect | kTakesChain | kTakesGridReflect,           // rtx_grid_reflect
};
static const unsigned kFamilyTakes[rtxplan::kShadeFamilies] = {
    kTakesShadow,                                              // rtx_shadow_shade
    kTakesLights,                                              // rtx_lights_shade
    kTakesShadow | kTakesReflect,                              // rtx_reflect_shade
    kTakesLights | kTakesReflect,                              // rtx_lights_reflect_shade
    kTakesLights | kTakesReflect | kTakesChain,                // rtx_lights_chain_shade
    kTakesLights | kTakesReflect | kTakesChain | kTakesDeep,   // rtx_lights_chain_shadow_shade
    kTakesLights | kTakesDark0,                                // rtx_grid_shade
    kTakesLights | kTakesReflect | kTakesDark0,                // rtx_grid_reflect_shade
    kTakesLights | kTakesReflect | kTakesChain | kTakesDark0,  // rtx_grid_chain_shade
    kTakesLights | kTakesReflect | kTakesChain | kTakesDeep | kTakesDark0, // rtx_grid_chain_shadow_shade
};

static bool tile_args_ok(const TileArgs* t, unsigned takes)
{
    const KArgs* a = t->a;
    if (t->cast != nullptr && (t->cast->sph == nullptr || t->cast->pl == nullptr || t->cast->gidx == nullptr)) return false; // (the flags: all three views or none)
    if ((takes & kTakesShadow) && t->shadow == nullptr) return false;
    if ((takes & kTakesLights) && (t->lights == nullptr || t->lights->lights.n == 0u || t->lights->lights.n > (uint32_t)rtxlights::kMaxLights)) return false;
    if ((takes & kTakesReflect) && t->reflect == nullptr) return false;
    if ((takes & kTakesChain) &&
        (t->chain == nullptr || t->chain->depth == 0u || t->chain->depth > (uint32_t)kMaxReflectDepth || t->chain->px != a->W * (a->row_end - a->row0))) {
        return false;
    }
    if ((takes & kTakesDeep) && (t->deep == nullptr || t->deep->dark == nullptr)) return false;
    if ((takes & kTakesDark0) && t->dark0 == nullptr) return false;
    if (takes & kTakesGrid) {
        const GridShadowArgs* gs = t->grid;
        if (gs == nullptr || gs->dark0 == nullptr || gs->fallback == nullptr || gs->grid.ok == 0u || a->ns == 0u) return false;
        if (t->reflect == nullptr || t->chain == nullptr || t->deep == nullptr) return false;
        if (gs->deep != 0u && !tile_args_ok(t, kTakesChain | kTakesDeep)) return false;
    }
    if (takes & kTakesGridReflect) {
        const GridReflectArgs* gr = t->grid_reflect;
        if (gr == nullptr || gr->pos_of_gidx == nullptr || gr->fallback == nullptr || gr->grid.ok == 0u || a->ns == 0u) return false;
    }
    return true;
}

// The arguments of the forms that read cones (rtx_scene_set_spots): the light set with the cones behind it, the one light with its
// own.  No cones given (a FIN form launched for the finishes alone): every light a point light.  Behind the cones the shadow-casting
// flags (rtx_scene_set_shadow_casting); none given: every object casts.
static SpotLightsArgs spot_lights_args(const TileArgs* t)
{
    SpotLightsArgs la;
    memset(&la, 0, sizeof la);
    static_cast<LightsArgs&>(la) = *t->lights;
    if (t->spots != nullptr) la.spots = *t->spots;
    if (t->cast != nullptr) la.cast = *t->cast; // (else nullptr: every object casts)
    return la;
}

static SpotShadowArgs spot_shadow_args(const TileArgs* t)
{
    SpotShadowArgs sa;
    memset(&sa, 0, sizeof sa);
    static_cast<ShadowArgs&>(sa) = *t->shadow;
    if (t->spots != nullptr) sa.spot = t->spots->spot[0];
    if (t->cast != nullptr) sa.cast = *t->cast;
    return sa;
}

// The largest argument block of any launch is rtx_grid_chain_shadow_shade's in its FIN form: it must fit the 4 KB a kernel may take.
static_assert(sizeof(KArgs) + sizeof(SpotLightsArgs) + sizeof(ReflectArgs) + sizeof(ChainArgs) + sizeof(ChainShadowArgs) + sizeof(const uint32_t*) + sizeof(PatternArgs) + 7 * 8 <= 4096,
              "rtx_grid_chain_shadow_shade's arguments, each aligned to 8, exceed the kernel-argument limit");
static_assert(sizeof(KArgs) + sizeof(SpotLightsArgs) + sizeof(ReflectArgs) + sizeof(ChainArgs) + sizeof(ChainShadowArgs) + sizeof(GridShadowArgs) + 6 * 8 <= 4096,
              "the arguments of rtx_grid_shadow's SPOT form, each aligned to 8, exceed the kernel-argument limit");

extern "C" const char* rtx_k_launch_pass(rtxplan::ShadePass pass, const TileArgs* t, void* stream_v, int* hip_error)
{
    using namespace rtx;
    *hip_error = 0;
    dim3 grid;
    if (pass == rtxplan::kPassNone || (unsigned)pass >= (unsigned)rtxplan::kShadePasses || !tile_grid(t->a, grid) || !tile_args_ok(t, kPassTakes[pass])) return nullptr;
    const dim3 block(kThreads, 1, 1);
    hipStream_t st = (hipStream_t)stream_v;
    const char* name = nullptr;
    switch (pass) {
    case rtxplan::kPassReflectHit:
        hipLaunchKernelGGL(rtx_reflect_hit, grid, block, 0, st, *t->a, *t->reflect);
        name = "rtx_reflect_hit";
        break;
    case rtxplan::kPassReflectChain:
        hipLaunchKernelGGL(rtx_reflect_chain, grid, block, 0, st, *t->a, *t->reflect, *t->chain);
        name = "rtx_reflect_chain";
        break;
    // (the two shadow passes: their SPOT form while some light of the set has a cone -- rtx_scene_set_spots -- or some object casts no
    // shadow -- rtx_scene_set_shadow_casting -- else the kernel they were)
    case rtxplan::kPassChainShadow:
        if (t->spots != nullptr || t->cast != nullptr) {
            hipLaunchKernelGGL(rtx_chain_shadow<true>, grid, block, 0, st, *t->a, spot_lights_args(t), *t->reflect, *t->chain, *t->deep);
            name = "rtx_chain_shadow<spot>";
        } else {
            hipLaunchKernelGGL(rtx_chain_shadow<false>, grid, block, 0, st, *t->a, *t->lights, *t->reflect, *t->chain, *t->deep);
            name = "rtx_chain_shadow";
        }
        break;
    case rtxplan::kPassGridShadow:
        if (t->spots != nullptr || t->cast != nullptr) {
            hipLaunchKernelGGL(rtx_grid_shadow<true>, grid, block, 0, st, *t->a, spot_lights_args(t), *t->reflect, *t->chain, *t->deep, *t->grid);
            name = "rtx_grid_shadow<spot>";
        } else {
            hipLaunchKernelGGL(rtx_grid_shadow<false>, grid, block, 0, st, *t->a, *t->lights, *t->reflect, *t->chain, *t->deep, *t->grid);
            name = "rtx_grid_shadow";
        }
        break;
    default:
        hipLaunchKernelGGL(rtx_grid_reflect, grid, block, 0, st, *t->a, *t->reflect, *t->chain, *t->grid_reflect);
        name = "rtx_grid_reflect";
        break;
    }
    *hip_error = (int)hipGetLastError();
    return name;
}

extern "C" const char* rtx_k_launch_shade(rtxplan::ShadeFamily family, const TileArgs* t, int mode, void* stream_v, int* hip_error)
{
    using namespace rtxplan;
    static const std::vector<ShadeNames> kNames = [] {
        std::vector<ShadeNames> v;
        for (int f = 0; f < kShadeFamilies; f++) v.emplace_back(shade_family_name((ShadeFamily)f));
        return v;
    }();
    *hip_error = 0;
    if ((unsigned)family >= (unsigned)kShadeFamilies || !tile_args_ok(t, kFamilyTakes[family])) return nullptr;
    const PatternArgs pa = t->pattern != nullptr ? *t->pattern : PatternArgs{nullptr, nullptr, nullptr, 0u, nullptr, nullptr};
    if ((pa.fin_sph == nullptr) != (pa.fin_pl == nullptr)) return nullptr; // (finishes: both orders or none)
    // the family's FIN form while some object has a finish of its own (rtx_scene_set_finish), else the form without: two kernels, not
    // one with a uniform test -- a kernel's registers are those of its hungrier path, and with both paths in one the chain's grid
    // families lost an occupancy step for every frame, finished or not (profiles/r36_finish_resource_usage.txt)
    // The FIN form also reads the cones of rtx_scene_set_spots, which travel behind the light set in its arguments (SpotLightsArgs,
    // SpotShadowArgs): one rich form per family, not a SPOT form beside FIN -- the render path hands it the finishes (the default
    // ones where no object has its own) whenever a light has a cone, so cones without finishes are refused here.
    // The shadow-casting flags (rtx_scene_set_shadow_casting) travel behind the cones, to the same form, under the same rule.
    if ((t->spots != nullptr || t->cast != nullptr) && pa.fin_sph == nullptr) return nullptr;
    const auto launch = [&](auto m, auto o, auto fin, dim3 grid, dim3 block) {
        constexpr int M = decltype(m)::value, O = decltype(o)::value;
        constexpr bool F = decltype(fin)::value;
        hipStream_t st = (hipStream_t)stream_v;
        // the light or the set as the form takes it: with the cones behind it (FIN), or as it is
        const auto one = [&]() -> ShadowArgsOf<F> {
            if constexpr (F) {
                return spot_shadow_args(t);
            } else {
                return *t->shadow;
            }
        };
        const auto set = [&]() -> LightsArgsOf<F> {
            if constexpr (F) {
                return spot_lights_args(t);
            } else {
                return *t->lights;
            }
        };
        switch (family) {
        case kShadowShade: hipLaunchKernelGGL((rtx::rtx_shadow_shade<M, O, F>), grid, block, 0, st, *t->a, one(), pa); break;
        case kLightsShade: hipLaunchKernelGGL((rtx::rtx_lights_shade<M, O, F>), grid, block, 0, st, *t->a, set(), pa); break;
        case kReflectShade: hipLaunchKernelGGL((rtx::rtx_reflect_shade<M, O, F>), grid, block, 0, st, *t->a, one(), *t->reflect, pa); break;
        case kLightsReflectShade: hipLaunchKernelGGL((rtx::rtx_lights_reflect_shade<M, O, F>), grid, block, 0, st, *t->a, set(), *t->reflect, pa); break;
        case kLightsChainShade: hipLaunchKernelGGL((rtx::rtx_lights_chain_shade<M, O, F>), grid, block, 0, st, *t->a, set(), *t->reflect, *t->chain, pa); break;
        case kLightsChainShadowShade:
            hipLaunchKernelGGL((rtx::rtx_lights_chain_shadow_shade<M, O, F>), grid, block, 0, st, *t->a, set(), *t->reflect, *t->chain, *t->deep, pa);
            break;
        case kGridShade: hipLaunchKernelGGL((rtx::rtx_grid_shade<M, O, F>), grid, block, 0, st, *t->a, set(), t->dark0, pa); break;
        case kGridReflectShade: hipLaunchKernelGGL((rtx::rtx_grid_reflect_shade<M, O, F>), grid, block, 0, st, *t->a, set(), *t->reflect, t->dark0, pa); break;
        case kGridChainShade: hipLaunchKernelGGL((rtx::rtx_grid_chain_shade<M, O, F>), grid, block, 0, st, *t->a, set(), *t->reflect, *t->chain, t->dark0, pa); break;
        default:
            hipLaunchKernelGGL((rtx::rtx_grid_chain_shadow_shade<M, O, F>), grid, block, 0, st, *t->a, set(), *t->reflect, *t->chain, *t->deep, t->dark0, pa);
            break;
        }
    };
    return launch_shade(t->a, mode, kNames[family], hip_error, [&](auto m, auto o, dim3 grid, dim3 block) {
        if (pa.fin_sph != nullptr) {
            launch(m, o, std::true_type{}, grid, block);
        } else {
            launch(m, o, std::false_type{}, grid, block);
        }
    });
}

// The fold of a supersampled launch (rtx_resolve_kernels.inc): a->W x (a->row_end - a->row0) cells of S x S samples each, read from
// `samples` (the sample frame's values, its row S a->row0 first) and written to a->out as `mode`'s records / words / values
// (a->compact 0 / 1 / 2).  Returns "rtx_resolve<S,RTX_K_mode>" with ",compact" or ",values" as the shade launches do, or nullptr
// when the launch is refused (S outside 2 .. 4, not a character mode, no cells, more workgroups than a grid holds).
extern "C" const char* rtx_k_launch_resolve(const KArgs* a, const void* samples, int S, int mode, void* stream_v, int* hip_error)
{
    using namespace rtx;
    struct Names {
        char s[3][5][3][64];
        Names()
        {
            static const char* const kMode[5] = {"RTX_K_BIT_ASCII", "RTX_K_BIT_PIXEL", "RTX_K_RGB_ASCII", "RTX_K_RGB_PIXEL", "RTX_K_RGB_NORMALS"};
            static const char* const kSuffix[3] = {"", ",compact", ",values"};
            for (int n = 0; n < 3; n++) {
                for (int m = 0; m < 5; m++) {
                    for (int o = 0; o < 3; o++) snprintf(s[n][m][o], sizeof s[n][m][o], "rtx_resolve<%d,%s%s>", n + 2, kMode[m], kSuffix[o]);
                }
            }
        }
    };
    static const Names kNames;
    static_assert(RTX_K_BIT_ASCII == 0 && RTX_K_RGB_NORMALS == 4 && kOutRecords == 0 && kOutCompact == 1 && kOutValues == 2, "names are indexed by mode and form");
    *hip_error = 0;
    const uint64_t cells = (uint64_t)a->W * (uint64_t)(a->row_end - a->row0), blocks = (cells + (uint64_t)kThreads - 1u) / (uint64_t)kThreads;
    if (S < 2 || S > 4 || mode < RTX_K_BIT_ASCII || mode > RTX_K_RGB_NORMALS || a->compact > 2u || samples == nullptr || a->row_end <= a->row0 || blocks == 0 ||
        blocks >= (1ull << 31)) {
        return nullptr;
    }
    const dim3 grid((uint32_t)blocks, 1, 1), block(kThreads, 1, 1);
    const ResolveArgs ra = {static_cast<const float4*>(samples)};
    hipStream_t st = (hipStream_t)stream_v;
    const auto with_out = [&](auto n, auto m) {
        constexpr int N = decltype(n)::value, M = decltype(m)::value;
        switch (a->compact) {
        case 0u: hipLaunchKernelGGL((rtx_resolve<N, M, kOutRecords>), grid, block, 0, st, *a, ra); break;
        case 1u: hipLaunchKernelGGL((rtx_resolve<N, M, kOutCompact>), grid, block, 0, st, *a, ra); break;
        default: hipLaunchKernelGGL((rtx_resolve<N, M, kOutValues>), grid, block, 0, st, *a, ra); break;
        }
    };
    const auto with_mode = [&](auto n) {
        switch (mode) {
        case RTX_K_BIT_ASCII: with_out(n, std::integral_constant<int, RTX_K_BIT_ASCII>{}); break;
        case RTX_K_BIT_PIXEL: with_out(n, std::integral_constant<int, RTX_K_BIT_PIXEL>{}); break;
        case RTX_K_RGB_ASCII: with_out(n, std::integral_constant<int, RTX_K_RGB_ASCII>{}); break;
        case RTX_K_RGB_PIXEL: with_out(n, std::integral_constant<int, RTX_K_RGB_PIXEL>{}); break;
        default: with_out(n, std::integral_constant<int, RTX_K_RGB_NORMALS>{}); break;
        }
    };
    switch (S) {
    case 2: with_mode(std::integral_constant<int, 2>{}); break;
    case 3: with_mode(std::integral_constant<int, 3>{}); break;
    default: with_mode(std::integral_constant<int, 4>{}); break;
    }
    *hip_error = (int)hipGetLastError();
    return kNames.s[S - 2][mode][a->compact];
}

extern "C" int rtx_k_launch_query(const QueryArgs* q, int kind, void* stream_v)
{
    if (q->n == 0u) return 0;
    const dim3 grid((q->n + (uint32_t)rtx::kThreads - 1u) / (uint32_t)rtx::kThreads), block(rtx::kThreads);
    if (kind == 0) {
        hipLaunchKernelGGL(rtx::rtx_query_grid, grid, block, 0, (hipStream_t)stream_v, *q);
    } else {
        hipLaunchKernelGGL(rtx::rtx_query_brute, grid, block, 0, (hipStream_t)stream_v, *q);
    }
    return (int)hipGetLastError();
}

extern "C" int rtx_k_launch_grid_build(const GridBuildArgs* b, int step, void* stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    const dim3 per_sphere((b->ns + (uint32_t)rtx::kThreads - 1u) / (uint32_t)rtx::kThreads), block(rtx::kThreads);
    switch (step) {
    case 0: hipLaunchKernelGGL(rtx::rtx_grid_bounds, dim3(1), block, 0, stream, *b); break;
    case 1: hipLaunchKernelGGL(rtx::rtx_grid_count, per_sphere, block, 0, stream, *b); break;
    case 2: hipLaunchKernelGGL(rtx::rtx_grid_scan, dim3(1), dim3(rtx::kScanThreads), 0, stream, *b); break;
    case 3: hipLaunchKernelGGL(rtx::rtx_grid_scatter, per_sphere, block, 0, stream, *b); break;
    case 4: {
        uint32_t blocks = (b->n_cells + 3u) / 4u;
        if (blocks > 4096u) blocks = 4096u;
        hipLaunchKernelGGL(rtx::rtx_grid_sort, dim3(blocks), block, 0, stream, *b);
        break;
    }
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

extern "C" int rtx_k_launch_pick_ray(const KArgs* a, uint32_t col, uint32_t row, void* d_ray, void* stream_v)
{
    hipLaunchKernelGGL(rtx::rtx_pick_ray, dim3(1), dim3(1), 0, (hipStream_t)stream_v, *a, col, row, (float4*)d_ray);
    return (int)hipGetLastError();
}

extern "C" int rtx_k_launch_bin_cells(const KArgs* a, unsigned splits, void* stream_v)
{
    return rtx::launch_bin_cells(a, splits, (hipStream_t)stream_v);
}

extern "C" int rtx_k_launch_order_tiles(const uint32_t* tile_cost, uint32_t n_tiles, uint32_t gx, uint32_t n_cu, uint32_t first_round,
                                        const uint32_t* base_order, uint32_t* tile_order, void* stream_v)
{
    return rtx::launch_order_tiles(tile_cost, n_tiles, gx, n_cu, first_round, base_order, tile_order, (hipStream_t)stream_v);
}

extern "C" int rtx_k_launch_balance_tiles(const uint32_t* tile_cost, uint32_t n_tiles, uint32_t gx, uint32_t n_cu, const uint32_t* prev_order,
                                          float* factor, int have_factor, int have_times, uint32_t* tile_order, void* stream_v)
{
    return rtx::launch_balance_tiles(tile_cost, n_tiles, gx, n_cu, prev_order, factor, have_factor, have_times, tile_order, (hipStream_t)stream_v);
}

extern "C" int rtx_k_launch_zero(void* p, size_t bytes, void* stream_v)
{
    if (bytes == 0) {
        return 0;
    }
    const size_t words = bytes / 4;
    size_t blocks = (words + rtx::kThreads - 1) / rtx::kThreads;
    if (blocks > 2048) {
        blocks = 2048;
    }
    hipLaunchKernelGGL(rtx::rtx_zero_fill, dim3((unsigned)blocks), dim3(rtx::kThreads), 0, (hipStream_t)stream_v, (uint32_t*)p, words);
    return (int)hipGetLastError();
}
