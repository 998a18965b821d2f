// rtx_resolve_kernels.inc -- the fold of a supersampled launch (RTX_OPT_SUPERSAMPLE, rtx.h), included into namespace rtx of
// rtx_kernels.hip after the shade kernels.  The launches before it are today's, for the S W x S H sample frame in values form
// (eight floats per sample: distance, shadingValue, normal.xyz, colour.xyz) into the render stream's sample buffer.  This one
// folds the S x S samples of every cell into one set of values and encodes it with encode_and_store, the one encoder.
//
// One thread per cell, cells numbered row by row over the launch's rows (x fastest), 256 per workgroup: console frames are narrow
// (160, 400 cells), so a workgroup spans rows instead of leaving most of a row-aligned one idle.  A cell's samples of one sub-row
// are 32 S contiguous bytes and neighbouring lanes continue them, so a wave reads 2 S float4s per lane and sub-row from one
// contiguous run of 2048 S bytes.  Every byte is read once, but a wave's load instructions share their 128-byte lines (one
// instruction takes 16 bytes of every 32 S), so the loads are plain: the L1 serves the rest of a line to the next instruction.
// Non-temporal loads, which bypass it, were measured and lost (1080p, fold alone: S = 2 86 us against 52, S = 4 657 against 236;
// profiles/r18_supersample_cost.txt); -DRTX_RESOLVE_NT_LOADS builds them for that A/B.  The fold is in registers, in the order
// rtx.h states: no operation may be added, removed or reordered (the GPU suite compares the values bit for bit with
// tests/restate_supersample.py).  32 S^2 bytes in, 4 to 32 bytes out per cell: bandwidth-bound.

struct ResolveArgs {
    const float4* samples;  // sample row S row0 of the sample frame at samples[0]; a row is S W samples of two float4s
};

typedef float resolve_v4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 resolve_load(const float4* p)
{
#ifdef RTX_RESOLVE_NT_LOADS // (the A/B build of the measurement above)
    const resolve_v4 v = __builtin_nontemporal_load(reinterpret_cast<const resolve_v4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}

template <int S, int MODE, int OUT>
__global__ __launch_bounds__(kThreads) void rtx_resolve(const KArgs a, const ResolveArgs ra)
{
    __shared__ uint32_t s_digits[256];
    __shared__ __attribute__((aligned(4))) uint8_t s_ramp[68];

    const uint32_t tid = threadIdx.x;
    s_digits[tid] = digits_word(tid);
    if (tid < 17u) {
        reinterpret_cast<uint32_t*>(s_ramp)[tid] = reinterpret_cast<const uint32_t*>(kRamp)[tid];
    }

    // the cell of this thread: a.W x (a.row_end - a.row0) cells, the frame's rows from a.row0
    const uint64_t cell = (uint64_t)blockIdx.x * (uint64_t)kThreads + tid;
    const uint64_t n_cells = (uint64_t)a.W * (uint64_t)(a.row_end - a.row0);
    const bool in_frame = cell < n_cells;
    const uint32_t lrow = in_frame ? (uint32_t)(cell / a.W) : 0u;
    const uint32_t col = in_frame ? (uint32_t)(cell - (uint64_t)lrow * a.W) : 0u;
    const bool newline_col = col + 1u == a.W;

    constexpr int N = S * S;
    float distance = kNoHit;
    float acc[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (in_frame && !newline_col) {
        // the samples (S col + i, S lrow + j), k = j S + i: all loads first, then the fold in k order
        const size_t sample_w = (size_t)S * a.W;
        const float4* p = ra.samples + ((size_t)S * lrow * sample_w + (size_t)S * col) * 2u;
        float4 lo[N], hi[N];
#pragma unroll
        for (int j = 0; j < S; j++) {
#pragma unroll
            for (int i = 0; i < S; i++) {
                lo[j * S + i] = resolve_load(p + ((size_t)j * sample_w + (size_t)i) * 2u);
                hi[j * S + i] = resolve_load(p + ((size_t)j * sample_w + (size_t)i) * 2u + 1u);
            }
        }
        bool any = false;
        float nearest = 0.0f;
#pragma unroll
        for (int k = 0; k < N; k++) {
            const bool vis = lo[k].x <= a.far;
            if (vis && (!any || lo[k].x < nearest)) nearest = lo[k].x;
            any = any || vis;
            acc[0] = acc[0] + (vis ? lo[k].y : 0.0f);
            acc[1] = acc[1] + (vis ? lo[k].z : 0.0f);
            acc[2] = acc[2] + (vis ? lo[k].w : 0.0f);
            acc[3] = acc[3] + (vis ? hi[k].x : 0.0f);
            acc[4] = acc[4] + (vis ? hi[k].y : 0.0f);
            acc[5] = acc[5] + (vis ? hi[k].z : 0.0f);
            acc[6] = acc[6] + (vis ? hi[k].w : 0.0f);
        }
        // (no visible sample: every sum is 0.0f + 0.0f, and the distance stays the miss distance)
        constexpr float kInvN = 1.0f / (float)N;
        if (any) distance = nearest;
#pragma unroll
        for (int v = 0; v < 7; v++) acc[v] = acc[v] * kInvN;
    }

    lds_barrier(); // the tables
    const Camera cam = tile_camera(a); // (the encoder reads its far distance)
    encode_and_store<MODE, OUT>(a, cam, s_digits, s_ramp, in_frame, newline_col, a.row0 + lrow, col, distance, v3(acc[1], acc[2], acc[3]), v3(acc[4], acc[5], acc[6]), acc[0]);
}
