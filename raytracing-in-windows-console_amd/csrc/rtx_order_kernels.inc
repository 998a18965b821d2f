// rtx_order_kernels.inc -- the passes that write a dispatch order: rtx_order_tiles, rtx_balance_tiles and the rules they are launched
// by.  Included into rtx_kernels.hip and into the direct check of these passes (tests/gpu_checks/sched_check.hip,
// tests/test_gpu_sched_check.py), inside namespace rtx, with BSTAMP and RTX_X_BALANCE_* of rtx_experiment.inc defined: both compile
// this text.

// rtx_order_tiles: the dispatch order of the next launches' macro tiles from the work estimates the workgroups of
// an earlier launch left in tile_cost.  One workgroup; a counting sort over 1024 cost classes (heaviest class first;
// the order within a class is whatever the atomics give -- any permutation renders the same frame, so only speed
// depends on it, and every tile receives exactly one rank by construction whatever tile_cost holds).
//
// (For grids of several dispatch rounds, and small ones; grids of one round go through rtx_balance_tiles below.)
// Why order at all: the first 7 workgroups per CU of a launch all become resident at once (1792 of the 2040 that
// config 2 had with 4 sub-tiles per workgroup), blocks b, b + n_cu, ... on one CU (observed: round-robin; nothing
// depends on it but speed), and finish when their CU has worked through whatever it was dealt.  In frame order the tiles of a CU differ by 3x in work and the expensive rows come last:
// the slowest CU takes a third longer than the average and the second-round workgroups start late and run long
// (profiles/r02_b_stamps_sub4.txt).  So: the tiles go out heaviest first, the first `first_round` of them dealt
// boustrophedon over the CUs (round k ascending for even k, descending for odd k) so that every CU's share
// carries the same work, and the light remainder fills the slots as they free up.
constexpr int kOrderThreads = 1024, kOrderBins = 1024;

// With `base` (the static XCD-aware order of a two-level grid: position -> packed tile, blocks b, b + 8, ... share an XCD and are
// handed whole cells, rtx_plan.hpp xcd_cell_order) the sort is PER LABEL: the tiles at the positions p = L mod 8 of `base` are
// put back, heaviest first, at the same positions -- every XCD keeps its cells (and its L2 their lists and spheres: config 5's
// trace kernel fetches 6 MB per launch this way and 19 MB under a plain heaviest-first order), within an XCD the heavy tiles
// come first.  1024 classes = 8 labels x 128 cost classes; a tile's position is 8 x (its rank within the label) + label.
__global__ __launch_bounds__(kOrderThreads) void rtx_order_tiles(const uint32_t* __restrict__ cost, uint32_t n, uint32_t gx, uint32_t n_cu,
                                                                  uint32_t first_round, const uint32_t* __restrict__ base, uint32_t* __restrict__ order)
{
    __shared__ uint32_t s_hist[kOrderBins];
    __shared__ uint32_t s_lo[kOrderThreads / 64], s_hi[kOrderThreads / 64];
    __shared__ uint32_t s_start[8];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (uint32_t i = tid; i < n; i += kOrderThreads) {
        const uint32_t c = cost[i];
        lo = c < lo ? c : lo;
        hi = c > hi ? c : hi;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0u) {
        s_lo[wave] = lo;
        s_hi[wave] = hi;
    }
    s_hist[tid] = 0u;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kOrderThreads / 64; k++) {
        lo = s_lo[k] < lo ? s_lo[k] : lo;
        hi = s_hi[k] > hi ? s_hi[k] : hi;
    }
    const uint64_t range = (uint64_t)(hi - lo) + 1u;
    auto bin_of = [&](uint32_t c) { return (uint32_t)(((uint64_t)(hi - c) * (uint64_t)kOrderBins) / range); }; // 0 = heaviest
    // per label: the class of the tile at position p of `base`
    auto tile_at = [&](uint32_t p) { const uint32_t packed = base[p]; return (packed >> 16) * gx + (packed & 0xffffu); };
    auto class_at = [&](uint32_t p) { return ((p & 7u) << 7) | (bin_of(cost[tile_at(p)]) >> 3); };
    for (uint32_t i = tid; i < n; i += kOrderThreads) {
        atomicAdd(&s_hist[base != nullptr ? class_at(i) : bin_of(cost[i])], 1u);
    }
    __syncthreads();
    // exclusive prefix sum over the classes (one per thread): wave scan, then the waves' totals
    const uint32_t mine = s_hist[tid];
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= (uint32_t)d) incl += o;
    }
    __syncthreads();
    if (lane == 63u) s_lo[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (int k = 0; k < kOrderThreads / 64; k++) {
        before += (uint32_t)k < wave ? s_lo[k] : 0u;
    }
    s_hist[tid] = before + incl - mine; // now: next free rank of the class
    if ((tid & 127u) == 0u) s_start[tid >> 7] = before + incl - mine; // (per label: where its ranks begin)
    __syncthreads();
    if (base != nullptr) {
        for (uint32_t p = tid; p < n; p += kOrderThreads) {
            const uint32_t label = p & 7u;
            const uint32_t rank = atomicAdd(&s_hist[class_at(p)], 1u) - s_start[label];
            order[8u * rank + label] = base[p]; // (the label's set has exactly as many tiles as there are positions = label mod 8)
        }
        return;
    }
    const uint32_t rounds = n_cu ? first_round / n_cu : 0u; // whole rounds dealt boustrophedon
    for (uint32_t i = tid; i < n; i += kOrderThreads) {
        const uint32_t rank = atomicAdd(&s_hist[bin_of(cost[i])], 1u);
        uint32_t blk = rank;
        if (n_cu && rank < rounds * n_cu) {
            const uint32_t k = rank / n_cu, c = rank - k * n_cu;
            blk = (k & 1u) ? k * n_cu + (n_cu - 1u - c) : rank;
        }
        const uint32_t by = i / gx, bx = i - by * gx;
        order[blk] = bx | (by << 16);
    }
}

// rtx_balance_tiles: the dispatch order for a tile grid whose workgroups are all resident at once (n <= slots per CU x
// n_cu; one workgroup, like rtx_order_tiles).  Then the blocks b, b + n_cu, b + 2 n_cu, ... share a compute unit
// (observed on every launch: profiles/r02_f_cu_balance.md; which physical CU varies, the groups do not), nothing is
// refilled, and the launch ends when the slowest group does -- in 1080p frame order a third later than the average
// one.  Two steps:
//   feedback  The instruction-count estimate ranks tiles well but is off by +-14 % on a group's sum (dependent
//             chains, the planes, divergence), while a group's duration repeats from launch to launch to 0.3 us.  So the
//             trace workgroups also leave their start and end times by dispatch position, and every tile carries a
//             correction factor: the tiles of a group that took longer than the mean group are scaled up, the others
//             down (damped, clamped), launch after launch.  cost' = (estimate + set-up) x factor.
//   dealing   The n - (rounds-1) n_cu lightest tiles are the last round (the hardware puts those blocks on groups
//             0, 1, ...).  The other rounds go heaviest first, and within a round the k-th heaviest tile goes to the
//             group with the k-th smallest sum so far.
// Any permutation renders the same frame; every position receives exactly one tile whatever the inputs hold (ranks come
// from counting, positions from ranks).
RTX_X_BALANCE_STAMPS();
// The pass runs beside the next frame's trace launch (a stream of its own), so it is shaped to fit into a slot that
// launch leaves free: 256 threads, the trace kernel's register budget, under 38 KB of LDS -- a CU holding six trace
// workgroups has room for exactly that.  (As one 1024-thread workgroup it needed a CU to itself and the frame beside it
// paid 20 us for the seven workgroups that CU could not take.)
constexpr int kBalanceMaxTiles = 2048;
constexpr int kBalanceThreads = 256;
constexpr int kBalancePerThread = kBalanceMaxTiles / kBalanceThreads;
constexpr int kBalanceBins = 1024;
constexpr uint32_t kCostSetup = 1800u; // per workgroup: tables, planes, staging (4 waves x ~4.5 passes' worth of time)

__global__ __launch_bounds__(kBalanceThreads, RTX_WAVES_PER_EU) void rtx_balance_tiles(const uint32_t* __restrict__ cost, uint32_t n, uint32_t gx,
                                                                                       uint32_t G, const uint32_t* prev_order, float* factor,
                                                                                       uint32_t have_factor, uint32_t have_times, uint32_t* order,
                                                                                       float damping, float max_step)
{
    // s_a: the estimates by tile, later the corrected costs by rank; s_b: the tile that ran at each position, later the
    // tile by rank
    __shared__ uint32_t s_a[kBalanceMaxTiles];
    __shared__ uint16_t s_b[kBalanceMaxTiles];
    __shared__ float s_f[kBalanceMaxTiles];        // factor by tile
    __shared__ float s_c[kBalanceMaxTiles];        // corrected cost by tile; before that, per group: earliest start, latest end
    int32_t* s_first = reinterpret_cast<int32_t*>(s_c);
    int32_t* s_last = s_first + kOrderThreads;
    static_assert(2 * kOrderThreads <= kBalanceMaxTiles, "the groups' times share s_c");
    __shared__ uint32_t s_hist[kBalanceBins];
    __shared__ float s_sum[kOrderThreads];         // per group: duration, then the sum dealt so far
    __shared__ float s_red[kBalanceThreads / 64];
    __shared__ uint32_t s_lo[kBalanceThreads / 64], s_hi[kBalanceThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    constexpr int kWaves = kBalanceThreads / 64;

    BSTAMP(0);
    for (uint32_t g = tid; g < (uint32_t)kOrderThreads; g += kBalanceThreads) {
        s_first[g] = 0x7fffffff;
        s_last[g] = (int32_t)0x80000000;
        s_hist[g] = 0u;
    }
    const uint32_t ref = have_times ? cost[n] : 0u;
    __syncthreads();
    // ---- everything this needs from memory, requested before anything is used (clamped indices instead of branches:
    // one round trip instead of eight); then the groups' first start and last end (a group's clocks are one XCD's:
    // only differences within a group are used)
    uint32_t c_in[kBalancePerThread], t0[kBalancePerThread], t1[kBalancePerThread], pk[kBalancePerThread];
    float f_in[kBalancePerThread];
#pragma unroll
    for (int q = 0; q < kBalancePerThread; q++) {
        const uint32_t i = tid + (uint32_t)q * kBalanceThreads;
        const uint32_t ii = i < n ? i : n - 1u;
        c_in[q] = cost[ii];
        t0[q] = have_times ? cost[n + ii] : 0u;
        t1[q] = have_times ? cost[2u * n + ii] : 0u;
        pk[q] = prev_order != nullptr ? prev_order[ii] : 0u;
        f_in[q] = have_factor ? factor[ii] : 1.0f;
    }
#pragma unroll
    for (int q = 0; q < kBalancePerThread; q++) {
        const uint32_t i = tid + (uint32_t)q * kBalanceThreads;
        if (i < n) {
            const uint32_t po = prev_order != nullptr ? (pk[q] >> 16) * gx + (pk[q] & 0xffffu) : i;
            s_a[i] = c_in[q];
            s_b[i] = (uint16_t)(po < n ? po : i);
            s_f[i] = (f_in[q] >= 0.5f && f_in[q] <= 2.0f) ? f_in[q] : 1.0f;
            if (have_times) {
                atomicMin(&s_first[i % G], (int32_t)(t0[q] - ref));
                atomicMax(&s_last[i % G], (int32_t)(t1[q] - ref));
            }
        }
    }
    __syncthreads();
    BSTAMP(1);
    // ---- feedback: how long each group took, against the mean
    float tot = 0.0f;
    for (uint32_t g = tid; g < G; g += kBalanceThreads) {
        float dur = 0.0f;
        if (have_times) {
            dur = (float)(s_last[g] - s_first[g]);
            dur = (dur > 0.0f && dur < 1.0e8f) ? dur : 0.0f; // (a second: nonsense)
        }
        s_sum[g] = dur;
        tot += dur;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) tot += __shfl_xor(tot, d);
    if (lane == 0u) s_red[wave] = tot;
    __syncthreads();
    tot = 0.0f;
#pragma unroll
    for (int k = 0; k < kWaves; k++) tot += s_red[k];
    const float mean = tot / (float)G;
    if (have_times && mean > 0.0f) {
        for (uint32_t p = tid; p < n; p += kBalanceThreads) { // a dispatch position; s_b: the tile that ran there
            const float d = s_sum[p % G];
            if (d > 0.0f) {
                float r = 1.0f + damping * (d / mean - 1.0f);
                r = r < 1.0f - max_step ? 1.0f - max_step : (r > 1.0f + max_step ? 1.0f + max_step : r);
                const uint32_t t = s_b[p];                      // (a permutation: every tile once)
                const float f = s_f[t] * r;
                s_f[t] = f < 0.5f ? 0.5f : (f > 2.0f ? 2.0f : f);
            }
        }
    }
    __syncthreads();
    BSTAMP(2);
    // ---- corrected costs; ranks by a counting sort over 1024 classes, heaviest first
    uint32_t lo = 0xffffffffu, hi = 0u;
    float total = 0.0f;
    for (uint32_t i = tid; i < n; i += kBalanceThreads) {
        const float f = s_f[i];
        factor[i] = f;
        const uint32_t c_in = s_a[i];
        const float c = (float)(c_in < (1u << 24) ? c_in + kCostSetup : (1u << 24)) * f;
        s_c[i] = c;
        total += c;
        const uint32_t u = (uint32_t)c;
        lo = u < lo ? u : lo;
        hi = u > hi ? u : hi;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
        total += __shfl_xor(total, d);
    }
    if (lane == 0u) {
        s_lo[wave] = lo;
        s_hi[wave] = hi;
        s_red[wave] = total;
    }
    __syncthreads();
    total = 0.0f;
#pragma unroll
    for (int k = 0; k < kWaves; k++) {
        lo = s_lo[k] < lo ? s_lo[k] : lo;
        hi = s_hi[k] > hi ? s_hi[k] : hi;
        total += s_red[k];
    }
    const float to_bin = (float)kBalanceBins / ((float)(hi - lo) + 1.0f);
    auto bin_of = [&](float c) { // 0 = heaviest
        const uint32_t b = (uint32_t)((float)(hi - (uint32_t)c) * to_bin);
        return b < (uint32_t)kBalanceBins ? b : (uint32_t)kBalanceBins - 1u;
    };
    // exclusive prefix sums over the 1024 classes in s_hist: four consecutive classes per thread, wave scan, wave totals
    auto scan_hist = [&]() {
        const uint32_t h0 = s_hist[4u * tid], h1 = s_hist[4u * tid + 1u], h2 = s_hist[4u * tid + 2u], h3 = s_hist[4u * tid + 3u];
        const uint32_t mine = h0 + h1 + h2 + h3;
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += o;
        }
        if (lane == 63u) s_lo[wave] = incl;
        __syncthreads();
        uint32_t before = incl - mine;
#pragma unroll
        for (int k = 0; k < kWaves; k++) {
            before += (uint32_t)k < wave ? s_lo[k] : 0u;
        }
        s_hist[4u * tid] = before;
        s_hist[4u * tid + 1u] = before + h0;
        s_hist[4u * tid + 2u] = before + h0 + h1;
        s_hist[4u * tid + 3u] = before + h0 + h1 + h2;
        __syncthreads();
    };
    for (uint32_t i = tid; i < n; i += kBalanceThreads) {
        atomicAdd(&s_hist[bin_of(s_c[i])], 1u);
    }
    __syncthreads();
    scan_hist();
    BSTAMP(3);
    for (uint32_t i = tid; i < n; i += kBalanceThreads) {
        const float c = s_c[i];
        const uint32_t rank = atomicAdd(&s_hist[bin_of(c)], 1u);
        s_a[rank] = __float_as_uint(c); // (the estimates are not needed any more, nor the positions)
        s_b[rank] = (uint16_t)i;
    }
    __syncthreads();
    BSTAMP(4);
    // ---- dealing
    auto put = [&](uint32_t pos, uint32_t rank) {
        const uint32_t t = s_b[rank];
        const uint32_t ty = t / gx, tx = t - ty * gx;
        order[pos] = tx | (ty << 16);
    };
    const uint32_t rounds = (n + G - 1u) / G, tail0 = (rounds - 1u) * G;
    for (uint32_t g = tid; g < G; g += kBalanceThreads) {
        float sum0 = 0.0f;
        if (tail0 + g < n) {
            sum0 = __uint_as_float(s_a[tail0 + g]);
            put(tail0 + g, tail0 + g);
        }
        s_sum[g] = sum0;
    }
    // Per round: rank the groups by their sums with the same counting sort (1024 classes over [0, 1.25 x the mean final
    // sum]: a class is 0.12 % of a group's work wide, far below what the estimates are good for; ties take the order the
    // atomics give), then the group with the k-th smallest sum takes the k-th heaviest tile of the round.
    const float sum_to_bin = total > 0.0f ? (float)kBalanceBins * (float)G / (1.25f * total) : 0.0f;
    auto sum_bin = [&](float v) {
        const uint32_t b = (uint32_t)(v * sum_to_bin);
        return b < (uint32_t)kBalanceBins ? b : (uint32_t)kBalanceBins - 1u;
    };
    BSTAMP(5);
    for (uint32_t r = 0; r + 1u < rounds; r++) {
        for (uint32_t k = tid; k < (uint32_t)kBalanceBins; k += kBalanceThreads) s_hist[k] = 0u;
        __syncthreads();
        for (uint32_t g = tid; g < G; g += kBalanceThreads) {
            atomicAdd(&s_hist[sum_bin(s_sum[g])], 1u);
        }
        __syncthreads();
        scan_hist();
        for (uint32_t g = tid; g < G; g += kBalanceThreads) {
            const float v = s_sum[g];
            const uint32_t k = atomicAdd(&s_hist[sum_bin(v)], 1u); // < G: the classes hold G groups in all
            put(r * G + g, r * G + k);
            s_sum[g] = v + __uint_as_float(s_a[r * G + k]);
        }
        __syncthreads();
    }
    BSTAMP(6);
}

// The launch rules of rtx_k_launch_order_tiles and rtx_k_launch_balance_tiles -- what they refuse, the clamp, the feedback's constants
// -- here so that the direct check (tests/gpu_checks/sched_check.hip) launches through them.
inline int launch_order_tiles(const uint32_t* tile_cost, uint32_t n_tiles, uint32_t gx, uint32_t n_cu, uint32_t first_round, const uint32_t* base_order,
                              uint32_t* tile_order, hipStream_t stream)
{
    if (n_tiles == 0 || gx == 0 || gx > 0xffffu || (n_tiles + gx - 1u) / gx > 0xffffu) {
        return (int)hipErrorInvalidValue;
    }
    if (first_round > n_tiles) first_round = n_tiles;
    hipLaunchKernelGGL(rtx_order_tiles, dim3(1), dim3(kOrderThreads), 0, stream, tile_cost, n_tiles, gx, n_cu, first_round, base_order, tile_order);
    return (int)hipGetLastError();
}

inline int launch_balance_tiles(const uint32_t* tile_cost, uint32_t n_tiles, uint32_t gx, uint32_t n_cu, const uint32_t* prev_order, float* factor,
                                int have_factor, int have_times, uint32_t* tile_order, hipStream_t stream)
{
    if (n_tiles == 0 || n_tiles > (uint32_t)kBalanceMaxTiles || gx == 0 || n_cu == 0 || n_cu > (uint32_t)kOrderThreads) {
        return (int)hipErrorInvalidValue;
    }
    RTX_X_BALANCE_DEBUG();
    // how much of a group's deviation from the mean duration goes into its tiles' factors per pass, and the largest step
    float damping = 0.7f, max_step = 0.18f;
    RTX_X_BALANCE_PARAMS(damping, max_step);
    hipLaunchKernelGGL(rtx_balance_tiles, dim3(1), dim3(kBalanceThreads), 0, stream, tile_cost, n_tiles, gx, n_cu, prev_order, factor, (uint32_t)have_factor,
                       (uint32_t)have_times, tile_order, damping, max_step);
    return (int)hipGetLastError();
}
