// rtx_bin_cells.inc -- the coarse-cell pass of two-level culling: rtx_bin_cells, bin_cells_of_block and the rule it is launched by.
// Included into rtx_kernels.hip and into the direct check of this pass (tests/gpu_checks/sched_check.hip,
// tests/test_gpu_sched_check.py), inside namespace rtx, after rtx_cull.hpp and rtx_workgroup.hpp: both compile this text.

// Level 1 of the two-level culling used for large scenes: the scene is binned into coarse cells (blocks of
// 2^gx x 2^gy macro tiles, a few hundred to a thousand of them) and every trace workgroup then stages its cell's
// list instead of the whole scene.  ONE launch, two levels inside it: workgroup (block, split) walks its share of the
// sphere array against the pyramid of a BLOCK of 4 x 4 cells -- the same conservative test as the per-tile one, on a
// larger rectangle -- gathers the survivors in LDS (hoisted centre and culling margin, as the REFINE pass of the trace
// kernel keeps them) and tests each of them against the 16 cell pyramids of the block, one (survivor, cell) pair
// per thread.  Sound level by level: a sphere that a pixel ray of a cell can hit can be hit by a ray of the
// cell's block.  Tests: blocks x spheres + 16 x survivors instead of cells x spheres.
//
// Lists are compact: cell c owns cell_cap entries (a few times the average; host: rtx_render_rows) and the
// workgroups append with one reservation per cell and flush -- atomicAdd on the cell's counter, which keeps
// counting past the capacity.  A trace workgroup that finds count > cell_cap stages the whole scene instead
// (always a superset), so a list that does not fit costs time, never a pixel.  The order of a list does not
// matter: the closest hit is the minimum of (t, creation index).
//
// The counters alternate between two buffers from launch to launch: this launch accumulates into
// cell_count_out and zeroes the 16 counters of its block in cell_count_zero, which the next launch on this
// stream accumulates into -- no memset between frames.
constexpr int kBlockCells = 16; // cells per block: 4 x 4
constexpr int kBinCap = 1024;   // block survivors gathered in LDS between cell phases

// Appends the block survivors [0, n) in s_rec / s_idx to the lists of the cells they can touch.
__device__ __forceinline__ void bin_cells_of_block(const KArgs& a, const float4* s_rec, const uint32_t* s_idx, uint32_t n, const float4 (*s_cellfr)[5],
                                                   uint32_t* s_cnt, uint32_t* s_base, uint32_t* s_pos, const uint32_t* s_cellid)
{
    const uint32_t tid = threadIdx.x;
    __syncthreads(); // survivors complete
    if (tid < (uint32_t)kBlockCells) {
        s_cnt[tid] = 0u;
        s_pos[tid] = 0u;
    }
    __syncthreads();
    // pass 1: the pairs' verdicts (kept in a bit mask: pair p = tid + 256 i is bit i) and the cells' counts
    const uint32_t pairs = n * (uint32_t)kBlockCells;
    unsigned long long keep = 0ull;
    for (uint32_t p = tid, i = 0; p < pairs; p += (uint32_t)kThreads, i++) {
        const uint32_t sv = p >> 4, c = p & 15u;
        if (s_cellid[c] == 0xffffffffu) {
            continue; // cell beyond the edge of the grid
        }
        const float4 r = s_rec[sv];
        bool out = false;
#pragma unroll
        for (int k = 0; k < 4; k++) { // (the four side planes: the block's survivors have passed the camera plane)
            const float4 nk = s_cellfr[c][k];
            out = out || (nk.x * r.x + nk.y * r.y + nk.z * r.z > r.w); // as tile_culls, margin in r.w (+inf: never)
        }
        if (!out) {
            keep |= 1ull << i;
            atomicAdd(&s_cnt[c], 1u);
        }
    }
    __syncthreads();
    if (tid < (uint32_t)kBlockCells && s_cnt[tid] != 0u) {
        s_base[tid] = atomicAdd(a.cell_count_out + s_cellid[tid], s_cnt[tid]); // one reservation per cell and flush
        // capacity feedback for the host (rtx_plan.hpp, cell_capacity_wanted): only lists past half their capacity report
        const uint32_t need = s_base[tid] + s_cnt[tid];
        if (a.cell_max_out != nullptr && need > (a.cell_cap >> 1)) atomicMax(a.cell_max_out, need);
    }
    __syncthreads();
    for (uint32_t p = tid, i = 0; p < pairs; p += (uint32_t)kThreads, i++) {
        if ((keep >> i) & 1ull) {
            const uint32_t sv = p >> 4, c = p & 15u;
            const uint32_t at = s_base[c] + atomicAdd(&s_pos[c], 1u);
            if (at < a.cell_cap) {
                a.cell_list_out[(size_t)s_cellid[c] * a.cell_cap + at] = a.sph_pos_of != nullptr ? a.sph_pos_of[s_idx[sv]] : s_idx[sv];
            }
        }
    }
    __syncthreads(); // the survivor buffer may be refilled
}

__global__ __launch_bounds__(kThreads) void rtx_bin_cells(const KArgs a)
{
    static_assert(kBinCap * kBlockCells <= 64 * kThreads, "a thread's pairs must fit the 64-bit verdict mask");
    __shared__ float4 s_rec[kBinCap];              // ox oy oz margin
    __shared__ uint32_t s_idx[kBinCap];
    __shared__ float4 s_cellfr[kBlockCells][5];
    __shared__ uint32_t s_cellid[kBlockCells];     // global cell number, or 0xffffffff beyond the grid
    __shared__ uint32_t s_cnt[kBlockCells], s_base[kBlockCells], s_pos[kBlockCells];
    __shared__ uint32_t s_wcnt[2][8];
    __shared__ float s_frustum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t tw = 1u << a.tile_log2w, th = (uint32_t)kThreads >> a.tile_log2w;
    const uint32_t nx = 1u << a.sub_log2nx, ny = a.nsub >> a.sub_log2nx;
    const uint32_t cw = (tw * nx) << a.cell_log2gx, ch = (th * ny) << a.cell_log2gy; // cell, pixels
    const uint32_t blocks_x = (a.cells_x + 3u) >> 2;
    const uint32_t bby = blockIdx.x / blocks_x, bbx = blockIdx.x - bby * blocks_x;   // this workgroup's block of cells

    Camera cam;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        cam.m[i] = a.m[i];
    }
    cam.ox = a.ox; cam.oy = a.oy; cam.oz = a.oz;
    cam.e1 = a.e1; cam.e2 = a.e2; cam.far = a.far;
    cam.fW = a.fW; cam.fH = a.fH;

    // pyramids: lanes 0..4 the block's five planes, lanes 5..84 plane k of cell c = (lane - 5) / 5
    if (tid < 5u + 5u * (uint32_t)kBlockCells) {
        if (tid < 5u) {
            const V3 n = tile_plane(a, cam, bbx * 4u * cw, a.row0 + bby * 4u * ch, 4u * cw, 4u * ch, tid);
            s_frustum[3 * tid + 0] = n.x;
            s_frustum[3 * tid + 1] = n.y;
            s_frustum[3 * tid + 2] = n.z;
        } else {
            const uint32_t q = tid - 5u, c = q / 5u, k = q - c * 5u;
            const uint32_t cx = bbx * 4u + (c & 3u), cy = bby * 4u + (c >> 2);
            const V3 n = tile_plane(a, cam, cx * cw, a.row0 + cy * ch, cw, ch, k);
            s_cellfr[c][k] = make_float4(n.x, n.y, n.z, 0.0f);
        }
    }
    if (tid < (uint32_t)kBlockCells) {
        const uint32_t cx = bbx * 4u + (tid & 3u), cy = bby * 4u + (tid >> 2);
        const bool valid = cx < a.cells_x && cy < a.cells_y;
        s_cellid[tid] = valid ? cy * a.cells_x + cx : 0xffffffffu;
        // the other counter buffer, for the next launch on this stream (one workgroup per block does it)
        if (valid && blockIdx.y == 0u && a.cell_count_zero != nullptr) {
            a.cell_count_zero[cy * a.cells_x + cx] = 0u;
        }
    }
    __syncthreads();
    TileFrustum fr;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        fr.n[k].x = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s_frustum[3 * k + 0])));
        fr.n[k].y = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s_frustum[3 * k + 1])));
        fr.n[k].z = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s_frustum[3 * k + 2])));
    }

    // The pass walks the scene array in creation order -- in the direction-sorted copy a block's spheres sit in one stretch, i.e.
    // in one workgroup's share: 36 us instead of 18 -- and translates the survivors to positions when it writes the lists.
    Items items;
    items.geom = a.sph_scene_geom;
    items.list = nullptr;
    items.count = a.ns;
    // this workgroup's share of the spheres: [lo, hi), a multiple of the step size except at the end
    const uint32_t ns = a.ns, splits = gridDim.y;
    const uint32_t steps = (ns + kChunk - 1) / kChunk;
    const uint32_t lo = (uint32_t)(((uint64_t)steps * blockIdx.y) / splits) * kChunk;
    const uint32_t hi_raw = (uint32_t)(((uint64_t)steps * (blockIdx.y + 1)) / splits) * kChunk;
    const uint32_t hi = hi_raw < ns ? hi_raw : ns;

    uint32_t total = 0, parity = 0;
    uint32_t k0, k1;
    float4 g0 = load_item(items, lo + tid, k0), g1 = load_item(items, lo + kThreads + tid, k1);
    for (uint32_t base = lo; base < hi; base += kChunk, parity ^= 1u) {
        const float4 g[2] = {g0, g1};
        const uint32_t kk[2] = {k0, k1};
        g0 = load_item(items, base + kChunk + tid, k0);
        g1 = load_item(items, base + kChunk + kThreads + tid, k1);
        if (total > (uint32_t)(kBinCap - kChunk)) {
            bin_cells_of_block(a, s_rec, s_idx, total, s_cellfr, s_cnt, s_base, s_pos, s_cellid);
            total = 0;
        }
        bool keep[2];
        float4 rec[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t k = base + (uint32_t)h * kThreads + tid;
            const float ox = cam.ox - g[h].x, oy = cam.oy - g[h].y, oz = cam.oz - g[h].z;
            const float oo = ox * ox + oy * oy + oz * oz;
            const float cc = oo - (g[h].w * g[h].w);
            float mg;
            bool inside;
            const bool culled = tile_culls_moving(fr, ox, oy, oz, oo, g[h].w, a.bin_theta, a.bin_delta, mg, inside);
            const bool outside = cc > 0.0f && !inside; // every camera the lists are for is strictly outside the sphere
            keep[h] = (k < hi) && !(outside && culled);
            // a camera inside or on the sphere: never culled, by any pyramid
            rec[h] = make_float4(ox, oy, oz, outside ? mg : __builtin_inff());
        }
        const unsigned long long m0 = __ballot(keep[0]), m1 = __ballot(keep[1]);
        if (lane == 0) {
            s_wcnt[parity][wave] = (uint32_t)__popcll(m0);
            s_wcnt[parity][4 + wave] = (uint32_t)__popcll(m1);
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        uint32_t before = 0, before1 = 0, first_total = 0, sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) {
            const uint32_t c0 = s_wcnt[parity][w], c1 = s_wcnt[parity][4 + w];
            first_total += c0;
            sum += c0 + c1;
            if (w < wave) {
                before += c0;
                before1 += c1;
            }
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        if (keep[0]) {
            const uint32_t pos = total + before + (uint32_t)__popcll(m0 & below);
            s_rec[pos] = rec[0];
            s_idx[pos] = kk[0];
        }
        if (keep[1]) {
            const uint32_t pos = total + first_total + before1 + (uint32_t)__popcll(m1 & below);
            s_rec[pos] = rec[1];
            s_idx[pos] = kk[1];
        }
        total = __builtin_amdgcn_readfirstlane(total + sum);
    }
    if (total) {
        bin_cells_of_block(a, s_rec, s_idx, total, s_cellfr, s_cnt, s_base, s_pos, s_cellid);
    }
}

// The launch rule of rtx_k_launch_bin_cells (one workgroup per block of 4 x 4 cells and split of the sphere array), here so that the
// direct check (tests/gpu_checks/sched_check.hip) launches through it.
inline int launch_bin_cells(const KArgs* a, unsigned splits, hipStream_t stream)
{
    const unsigned blocks = ((a->cells_x + 3u) >> 2) * ((a->cells_y + 3u) >> 2);
    hipLaunchKernelGGL(rtx_bin_cells, dim3(blocks, splits, 1), dim3(kThreads), 0, stream, *a);
    return (int)hipGetLastError();
}
