// rtx_post_kernels.inc -- the device code of rtx_post.hip (included there, once): the physics step (UpdateObjects), the sphere gather
// of the direction-sorted scene copy, the xterm-256 mapper over a range, and Minimize from records or from pixel words -- as one launch
// (rtx_min_fused, with the look-back it finds its offsets by) or as the chain rtx_min_count / rtx_min_offsets / rtx_min_scatter.  The
// host side (buffers, launches, the Update entry points): rtx_post.hip.  Delta frames (rtx_delta_words) are a third slot source of the
// same Minimize kernels, DeltaSource, over two frames of pixel words; half-block frames (rtx_half_words) a fourth, HalfSource, over
// pairs of pixel rows; their delta frames (rtx_half_delta_words) a fifth, HalfDeltaSource, over two such frames.
namespace rtx {

constexpr int kThreads = 256;

// ---------------------------------------------------------------- UpdateObjects
// Sphere::Update, Sphere.cu:15-23 (long double is double in device code); Plane::Update is a no-op
// (Plane.cu:14-18).  One thread per sphere with a launch shape that is valid for any count: the
// reference's block of `count` threads stops launching past 1024 objects (SURVEY App. E-5).
__global__ __launch_bounds__(kThreads) void rtx_update_spheres(float4* geom, float4* motion, uint32_t ns, double dt, float4* sorted_geom,
                                                               const uint32_t* pos_of)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= ns) {
        return;
    }
    float4 g = geom[i];
    float4 mv = motion[i];
    int mover = (int)__float_as_uint(mv.x);
    const float speed = mv.y;
    // m_center.y += speed * mover * dt;
    g.y = (float)((double)g.y + (double)(speed * (float)mover) * dt);
    if (g.y < -10.0f || g.y > 10.0f) {
        const float r = g.y < -10.0f ? -10.0f : g.y; // MyMath::Clamp, MyMath.cu:29-34
        g.y = r > 10.0f ? 10.0f : r;
        mover *= -1;
    }
    mv.x = __uint_as_float((uint32_t)mover);
    geom[i] = g;
    motion[i] = mv;
    if (sorted_geom != nullptr) {
        sorted_geom[pos_of[i]] = g; // the direction-sorted copy staging reads (rtx_sort_scene) moves with it
    }
}

// ---------------------------------------------------------------- rtx_scene_set_spheres
// Object3D::SetMiddlePos (Object3D.cu:34), which the reference never calls after upload, for a run of spheres: sphere first + j
// takes centre, radius and colour of row j of `rows` (7 floats, cx cy cz r R G B; 4-byte aligned device memory).  One sphere per
// thread; a block's rows are loaded as consecutive dwords into LDS first (a lane's own seven are 28 bytes apart in memory; in LDS
// the stride of 7 dwords is odd against 64 banks: no conflicts).  The .w words of color / od (the creation index) stay; od is the
// IEEE division rtx_scene_add_sphere does on the host (-fno-fast-math: the compiler's `/`, tests/test_gpu_div.py).
// The old geometry lives only here (physics moves it), so the bound on how far anything moved is formed here as well:
// result[0] = the bits of the largest |new centre - old centre|, formed in double and rounded UP to float (atomicMax on the bits:
// order-preserving for floats >= 0), result[1] = flags ORed over the spheres: bit 0 a radius changed (NaN counts), bit 1 a move
// that is no finite float (it then adds 0 to the maximum), bit 2 a new cy outside [-10, 10] (NaN counts).  Both zeroed by the host.
__global__ __launch_bounds__(kThreads) void rtx_write_spheres(const float* rows, uint32_t first, uint32_t n, float4* geom, float4* color, float4* od,
                                                              float4* sorted_geom, float4* sorted_od, const uint32_t* pos_of, uint32_t* result)
{
    __shared__ float s_rows[kThreads * 7];
    const uint32_t base = blockIdx.x * kThreads;
    const uint32_t here = n - base < (uint32_t)kThreads ? n - base : (uint32_t)kThreads; // (the tail block)
    const float* src = rows + (size_t)base * 7u;
    for (uint32_t k = threadIdx.x; k < here * 7u; k += kThreads) {
        s_rows[k] = src[k];
    }
    __syncthreads();
    uint32_t move_bits = 0u, flags = 0u;
    if (threadIdx.x < here) {
        const uint32_t i = first + base + threadIdx.x;
        const float* v = s_rows + threadIdx.x * 7u;
        const float4 g = make_float4(v[0], v[1], v[2], v[3]);
        const float4 old = geom[i];
        const double dx = (double)g.x - (double)old.x, dy = (double)g.y - (double)old.y, dz = (double)g.z - (double)old.z;
        // a few double ulps up, so that whatever the last bit of the device's sqrt, the float below is no less than the true length
        const double move = sqrt(dx * dx + dy * dy + dz * dz) * (1.0 + 0x1p-50);
        float up = (float)move;
        if ((double)up < move) {
            up = __uint_as_float(__float_as_uint(up) + 1u); // (up >= 0: the next float up; the largest float goes to +inf)
        }
        if (!(move == move) || !(up < __uint_as_float(0x7f800000u))) {
            flags |= 2u;
        } else {
            move_bits = __float_as_uint(up);
        }
        flags |= (g.w != old.w) ? 1u : 0u;
        flags |= (g.y >= -10.0f && g.y <= 10.0f) ? 0u : 4u;
        float4 c = color[i], o = od[i];
        c.x = v[4];
        c.y = v[5];
        c.z = v[6];
        o.x = v[4] / 255.0f;
        o.y = v[5] / 255.0f;
        o.z = v[6] / 255.0f;
        geom[i] = g;
        color[i] = c;
        od[i] = o;
        if (sorted_geom != nullptr) {
            const uint32_t p = pos_of[i];
            float4 so = sorted_od[p];
            so.x = o.x;
            so.y = o.y;
            so.z = o.z;
            sorted_geom[p] = g; // the direction-sorted copy staging reads (rtx_sort_scene) takes the edit too
            sorted_od[p] = so;
        }
    }
    // one atomic pair per wave (wave64: kThreads is a multiple of 64 and no lane has left)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t m = (uint32_t)__shfl_xor((int)move_bits, s);
        flags |= (uint32_t)__shfl_xor((int)flags, s);
        move_bits = m > move_bits ? m : move_bits;
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (move_bits != 0u) atomicMax(&result[0], move_bits);
        if (flags != 0u) atomicOr(&result[1], flags);
    }
}

// ---------------------------------------------------------------- rtx_scene_remove_objects
// No reference counterpart (Scene3D.h:15-25 creates objects, Scene3D::CleanUp frees all of them at once).  Compacts the four
// float4 arrays of one kind -- spheres: plain0/1 = geom, motion, idx0/1 = color, od; planes: plain0/1 = a, b, idx0/1 = c, od; the
// idx arrays carry the creation index in .w -- OUT OF PLACE: one source object per thread; the survivor of local index k goes to
// k' = k - |{removed locals < k}| of the destination set with g' = g - |{removed creation indices < g}| in its two .w words, every
// other bit as it was (pure moves).  The destinations of one thread are the sources of another and a launch has no order, hence
// the second set; the host swaps the sets afterwards.  Both lists are ascending, in global memory (L2-resident: 4 bytes per
// removed object) and searched by bisection: about log2 |R| dependent loads per thread against the 8 x 16 bytes it moves.
__device__ __forceinline__ uint32_t count_below(const uint32_t* list, uint32_t n, uint32_t v)
{
    uint32_t lo = 0u, hi = n; // the first position whose entry is >= v
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (list[mid] < v) {
            lo = mid + 1u;
        } else {
            hi = mid;
        }
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void rtx_compact_objects(const float4* plain0, const float4* plain1, const float4* idx0, const float4* idx1,
                                                                float4* out_plain0, float4* out_plain1, float4* out_idx0, float4* out_idx1,
                                                                uint32_t count, const uint32_t* removed_gidx, uint32_t n_gidx,
                                                                const uint32_t* removed_local, uint32_t n_local)
{
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= count) return;
    const uint32_t below = count_below(removed_local, n_local, k);
    if (below < n_local && removed_local[below] == k) return; // removed
    const float4 i0 = idx0[k], i1 = idx1[k], p0 = plain0[k], p1 = plain1[k];
    const uint32_t g = __float_as_uint(i0.w);
    const float w = __uint_as_float(g - count_below(removed_gidx, n_gidx, g));
    const uint32_t to = k - below; // (<= k < count: inside every destination array, which holds at least `count`)
    out_plain0[to] = p0;
    out_plain1[to] = p1;
    out_idx0[to] = make_float4(i0.x, i0.y, i0.z, w); // (built anew: with i0.w = w this compiler's alloca promotion gave the kernel 6144 bytes of LDS, profiles/r14_scene_remove_resource_usage.txt)
    out_idx1[to] = make_float4(i1.x, i1.y, i1.z, w);
}

// sorted[p] = geom[order[p]]: the direction-sorted copy of the sphere array, from the live one.
__global__ __launch_bounds__(kThreads) void rtx_gather_spheres(const float4* geom, const float4* od, const uint32_t* order, float4* sorted_geom,
                                                               float4* sorted_od, uint32_t ns)
{
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p < ns) {
        sorted_geom[p] = geom[order[p]];
        sorted_od[p] = od[order[p]];
    }
}

// ---------------------------------------------------------------- ansi256_from_rgb over a range of inputs
// The mapper of the 8-bit trace kernels (rtx_device.hpp, ANSIRGB.h:141-189) applied to packed 0xRRGGBB values
// first .. first+count-1, four per thread, one dword store each.
__global__ __launch_bounds__(kThreads) void rtx_ansi_map(uint32_t first, uint64_t count, const uint8_t* grey, uint8_t* out)
{
    const uint64_t i0 = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * 4u;
    if (i0 >= count) {
        return;
    }
    uint32_t v[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t rgb = first + (uint32_t)i0 + k;
        v[k] = ansi256_from_rgb((rgb >> 16) & 255u, (rgb >> 8) & 255u, rgb & 255u, grey);
    }
    if (i0 + 4u <= count && (((uintptr_t)(out + i0)) & 3u) == 0u) {
        *reinterpret_cast<uint32_t*>(out + i0) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
        for (uint32_t k = 0; k < 4u && i0 + k < count; k++) {
            out[i0 + k] = (uint8_t)v[k];
        }
    }
}

// ---------------------------------------------------------------- Minimize
//
// The reference scans the frame byte by byte on one CPU thread.  Restated per slot (a slot is one
// S-byte record position; W slots per row, the last one being the row's NUL column):
//   * NUL-column slot           -> emits '\n'                        (RayTracingManager.cu:223-239)
//   * slot starting with ESC    -> emits the whole record if its colour digits differ from the
//                                  colour of the previous ESC slot in scan order (rows included),
//                                  else only its last byte (the glyph)   (:193-220)
//   * any other slot (all NUL)  -> emits nothing                     (:241-245)
// "latestColor" only moves when the colour differs, so comparing with the previous ESC slot is the
// same test.  Output offsets are an exclusive prefix sum of the emitted lengths.
//
// A block owns kSlotsPerBlock consecutive slots, a thread four consecutive ones.  The kernels (rtx_min_count, rtx_min_scatter,
// rtx_min_fused, at the end) are written once over a slot source, one per input form (RecordSource, WordSource), which
//   * stages the block's slots and the two slots before them in LDS (where a rendered frame's previous ESC slot always is),
//   * gives the emitted length of a slot (and keeps what emit() needs of it in an Item),
//   * writes a slot's emitted bytes -- the whole record, its glyph alone or '\n' -- into the block's LDS image (stage_tables()
//     first fills what that takes besides the slot),
//   * and says how much LDS the block's buffer takes: kStage for the staged slots and the scan's partial sums (at kWave), kBytes
//     with the image, which is built over the staged slots once every thread holds its own.
constexpr int kPerThread = 4;
constexpr int kSlotsPerBlock = kThreads * kPerThread; // 1024

template <int S>
struct Slot {
    uint32_t w[S / 4];
};

template <int S>
__device__ __forceinline__ bool same_colour(const Slot<S>& a, const Slot<S>& b)
{
    if (S == 12) {
        // bytes 7, 8, 9
        return ((a.w[1] ^ b.w[1]) & 0xff000000u) == 0u && ((a.w[2] ^ b.w[2]) & 0x0000ffffu) == 0u;
    }
    // bytes 7-9, 11-13, 15-17
    return ((a.w[1] ^ b.w[1]) & 0xff000000u) == 0u && ((a.w[2] ^ b.w[2]) & 0xff00ffffu) == 0u &&
           ((a.w[3] ^ b.w[3]) & 0xff00ffffu) == 0u && ((a.w[4] ^ b.w[4]) & 0x0000ffffu) == 0u;
}

template <int S>
__device__ __forceinline__ Slot<S> load_slot(const uint8_t* p)
{
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    Slot<S> s;
#pragma unroll
    for (int k = 0; k < S / 4; k++) {
        s.w[k] = q[k];
    }
    return s;
}

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* s_wave, uint32_t& block_total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= (uint32_t)d) {
            incl += o;
        }
    }
    if (lane == 63u) {
        s_wave[wave] = incl;
    }
    __syncthreads();
    uint32_t base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; k++) {
        const uint32_t t = s_wave[k];
        base += (uint32_t)k < wave ? t : 0u;
        total += t;
    }
    __syncthreads();
    block_total = total;
    return base + incl - v;
}

// Column of slot base + li0, this thread's first: the block's first column by one scalar 64-bit division (the block index is uniform),
// the thread's by a 32-bit one (a 64-bit division per thread is ~100 instructions, a third of what this pass executes).
__device__ __forceinline__ uint32_t first_column(uint64_t base, uint32_t W, uint32_t li0)
{
    // (a 64-bit remainder is ~130 instructions, a tenth of what a wave of the one-launch form executes: 32-bit where the slot fits)
    const uint32_t col0 = (uint32_t)__builtin_amdgcn_readfirstlane((base >> 32) == 0u ? (uint32_t)base % W : (uint32_t)(base % W));
    return (col0 + li0) % W; // (col0 < W < 2^31 and li0 < 1024: no overflow)
}

// ---- records: S = 12 or 20 bytes per slot.  The block's bytes (plus a halo of the two slots before it) are brought into LDS with
// coalesced 16-byte loads; slots are then read from LDS at their 12/20-byte stride (3 or 5 dwords).
constexpr int kHaloOff = 48; // LDS byte offset of the block's first slot: 16-byte aligned, room for 2 x 20 halo bytes
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;

// The previous ESC slot of slot g is not among the two staged before it (a frame that was only partly rendered: empty slots in
// between): walk back through global memory.  Rare, and kept out of line so that the passes' straight-line code stays short.
template <int S>
__device__ __noinline__ uint32_t record_length_walk(const uint8_t* __restrict__ in, uint64_t g, uint32_t W, Slot<S> rec)
{
    uint64_t j = g;
    while (j > 0) {
        --j;
        if ((uint32_t)(j % W) == W - 1u) {
            continue;
        }
        if (in[j * S] == 0x1bu) {
            return same_colour<S>(rec, load_slot<S>(in + j * S)) ? 1u : (uint32_t)S;
        }
    }
    return (uint32_t)S; // first pixel of the frame
}

template <int S>
struct RecordSource {
    typedef uint8_t Elem;  // the input
    typedef const uint8_t* __restrict__ In; // ... as the kernels receive it
    typedef Slot<S> Item;  // what a thread keeps of a slot
    static constexpr uint32_t kS = S;
    static constexpr uint32_t kWave = kHaloOff + kSlotsPerBlock * S;
    static constexpr uint32_t kStage = kWave + 16;
    static constexpr uint32_t kBytes = kStage;

    static __device__ __forceinline__ void stage(const uint8_t* __restrict__ in, uint64_t base, uint64_t n_slots, uint32_t, uint8_t* s, uint32_t)
    {
        const uint64_t b0 = base * S;
        const uint64_t total_bytes = n_slots * S;
        const uint64_t b1 = b0 + (uint64_t)kSlotsPerBlock * S < total_bytes ? b0 + (uint64_t)kSlotsPerBlock * S : total_bytes;
        const uint32_t nbytes = (uint32_t)(b1 - b0); // multiple of 4; in + b0 is 16-byte aligned (1024 S is a multiple of 16)
        const uint32_t n16 = nbytes / 16u;
        const uint4* src = reinterpret_cast<const uint4*>(in + b0);
        uint4* dst = reinterpret_cast<uint4*>(s + kHaloOff);
        for (uint32_t i = threadIdx.x; i < n16; i += kThreads) {
            dst[i] = src[i];
        }
        // tail dwords (when the frame ends inside this block) and the halo
        const uint32_t* src32 = reinterpret_cast<const uint32_t*>(in + b0);
        uint32_t* dst32 = reinterpret_cast<uint32_t*>(s + kHaloOff);
        for (uint32_t i = n16 * 4u + threadIdx.x; i < nbytes / 4u; i += kThreads) {
            dst32[i] = src32[i];
        }
        if (threadIdx.x < 2u * S / 4u) {
            const uint32_t hd = threadIdx.x; // dword of the halo, counted from its start
            uint32_t v = 0u;
            if (b0 >= 2u * S) {
                v = reinterpret_cast<const uint32_t*>(in + b0 - 2u * S)[hd];
            } else if (b0 >= S && hd >= S / 4u) {
                v = reinterpret_cast<const uint32_t*>(in + b0 - S)[hd - S / 4u];
            }
            reinterpret_cast<uint32_t*>(s + kHaloOff - 2 * S)[hd] = v;
        }
    }

    static __device__ __forceinline__ void stage_tables() {}
    static In input(const void* data, const void*, void*) { return (In)data; }
    static __device__ __forceinline__ void tally_put(const uint32_t*) {}
    static __device__ __forceinline__ void tally_add(In) {}

    // Emitted length of slot g (column col, staged at li); `rec` receives the record when the slot is a pixel.
    static __device__ __forceinline__ uint32_t length(const uint8_t* __restrict__ in, const uint8_t* s, uint64_t g, int li, uint32_t col, uint32_t W, uint32_t,
                                                      Slot<S>& rec)
    {
        if (col == W - 1u) {
            return 1u; // newline
        }
        rec = load_slot<S>(s + kHaloOff + li * S);
        if ((rec.w[0] & 0xffu) != 0x1bu) {
            return 0u;
        }
        if (g == 0) {
            return (uint32_t)S; // first pixel of the frame
        }
        // previous ESC slot: slot g-1, or g-2 when g-1 is the previous row's NUL column
        const int back = col == 0u ? 2 : 1;
        if (g >= (uint64_t)back) {
            const Slot<S> prev = load_slot<S>(s + kHaloOff + (li - back) * S);
            if ((prev.w[0] & 0xffu) == 0x1bu) {
                return same_colour<S>(rec, prev) ? 1u : (uint32_t)S;
            }
        }
        return record_length_walk<S>(in, g, W, rec);
    }

    static __device__ __forceinline__ void emit(uint8_t* dst, uint32_t len, bool newline, const Slot<S>& rec)
    {
        if (len == (uint32_t)S) {
#pragma unroll
            for (int q = 0; q < S / 4; q++) {
                *reinterpret_cast<u32_unaligned*>(dst + 4 * q) = rec.w[q];
            }
        } else if (len == 1u) {
            dst[0] = newline ? (uint8_t)'\n' : (uint8_t)(rec.w[S / 4 - 1] >> 24);
        }
    }
};

// ---- compact pixel words
//
// The 4-byte pixel words the trace kernels can store instead of records (RTX_RENDER_COMPACT, rtx.h): a word carries everything its
// record is made of, so the pass reads 4 bytes per pixel where the record form reads 12 or 20 -- twice.  rtx_update traces words and
// minimises from them: 8.3 MB written and 2 x 8.3 MB read per 1080p frame instead of 41.5 MB and 2 x 41.5 MB (the full-size records
// never exist), and a device group gathers the words it minimises from (no expansion).  Slot rules as above, stated on words:
//   * column W-1                          -> '\n'
//   * word 0xffffffff elsewhere           -> an empty slot (all NUL as a record): emits nothing, is not an ESC slot
//   * any other word (0 = miss)           -> an ESC slot: its record is record_words<MODE>(word); the colour Minimize compares
//     (bytes 7-9 [, 11-13, 15-17] of the record: the decimal digits) is a function of the word's colour bytes alone -- the
//     digits of (r, g, b) or of the xterm index; a miss carries the digits of (0, 0, 0) resp. of index 16 (App. B) -- so
//     "same colour digits" is "same colour key".
constexpr uint32_t kNoWord = 0xffffffffu; // = kCompactNewline

template <int MODE>
__device__ __forceinline__ uint32_t colour_key(uint32_t w)
{
    constexpr bool kRgb = (MODE == RTX_K_RGB_ASCII || MODE == RTX_K_RGB_PIXEL || MODE == RTX_K_RGB_NORMALS);
    return kRgb ? (w & 0x00ffffffu) : (w != 0u ? (w & 0xffu) : 16u);
}

// As record_length_walk.  `lead`: how many words BEFORE words[0] exist and belong to the same frame (0, or the W words of the row
// above a slab: a rank of a device group minimises its own rows and needs the last pixel of the row before them; rtx_update on a
// group, RTX_OPT_GROUP_UPDATE).
template <int MODE>
__device__ __noinline__ uint32_t word_length_walk(const uint32_t* __restrict__ words, uint64_t g, uint32_t W, uint32_t w, uint32_t lead)
{
    constexpr uint32_t S = (MODE == RTX_K_RGB_ASCII || MODE == RTX_K_RGB_PIXEL || MODE == RTX_K_RGB_NORMALS) ? 20u : 12u;
    int64_t j = (int64_t)g;
    while (j > -(int64_t)lead) {
        --j;
        if ((uint32_t)((uint64_t)(j + (int64_t)lead) % W) == W - 1u) { // (lead is a multiple of W)
            continue;
        }
        const uint32_t pw = words[j];
        if (pw != kNoWord) {
            return colour_key<MODE>(pw) == colour_key<MODE>(w) ? 1u : S;
        }
    }
    return S;
}

// The block's buffer: s_w[0..1] = the two words before the block's first slot (kNoWord where the frame begins), s_w[2 + li] = word
// of slot base + li, the scan's partial sums behind them.  The digit table of record_words is an LDS array of its own (apart from
// the image, its loads are free to move past the image's stores).
template <int MODE>
struct WordSource {
    typedef uint32_t Elem;
    typedef const uint32_t* __restrict__ In;
    typedef uint32_t Item;
    static constexpr uint32_t kS = (MODE == RTX_K_RGB_ASCII || MODE == RTX_K_RGB_PIXEL || MODE == RTX_K_RGB_NORMALS) ? 20u : 12u;
    static constexpr uint32_t kWave = (2 + kSlotsPerBlock + 2) * 4;
    static constexpr uint32_t kStage = kWave + (kThreads / 64) * 4;
    static constexpr uint32_t kBytes = kSlotsPerBlock * kS;
    static_assert(kStage <= kBytes, "words + partial sums fit the image's space");

    static __device__ __forceinline__ uint32_t* digits()
    {
        __shared__ uint32_t s_digits[256];
        return s_digits;
    }

    static __device__ __forceinline__ void stage(const uint32_t* __restrict__ words, uint64_t base, uint64_t n_slots, uint32_t lead, uint8_t* s, uint32_t)
    {
        uint32_t* s_w = reinterpret_cast<uint32_t*>(s);
        const uint32_t tid = threadIdx.x;
        const uint64_t g0 = base + (uint64_t)tid * kPerThread;
        if (g0 + kPerThread <= n_slots && ((uintptr_t)(words + g0) & 15u) == 0u) {
            const uint4 v = *reinterpret_cast<const uint4*>(words + g0);
            s_w[2 + tid * kPerThread + 0] = v.x;
            s_w[2 + tid * kPerThread + 1] = v.y;
            s_w[2 + tid * kPerThread + 2] = v.z;
            s_w[2 + tid * kPerThread + 3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < kPerThread; k++) {
                s_w[2 + tid * kPerThread + k] = g0 + k < n_slots ? words[g0 + k] : kNoWord;
            }
        }
        if (tid < 2u) {
            s_w[tid] = base + tid + lead >= 2u ? words[(int64_t)(base + tid) - 2] : kNoWord;
        }
    }

    static __device__ __forceinline__ void stage_tables() { digits()[threadIdx.x] = digits_word(threadIdx.x); }
    static In input(const void* data, const void*, void*) { return (In)data; }
    static __device__ __forceinline__ void tally_put(const uint32_t*) {}
    static __device__ __forceinline__ void tally_add(In) {}

    // Emitted length of slot g (column col, staged at s_w[2 + li]); `w` receives its word.  Selects, and one branch for the rare walk.
    static __device__ __forceinline__ uint32_t length(const uint32_t* __restrict__ words, const uint8_t* s, uint64_t g, int li, uint32_t col, uint32_t W,
                                                      uint32_t lead, uint32_t& w)
    {
        const uint32_t* s_w = reinterpret_cast<const uint32_t*>(s);
        w = s_w[2 + li];
        // previous ESC slot: slot g-1, or g-2 when g-1 is the previous row's last column (both staged: s_w[0..1] precede the block)
        const int back = col == 0u ? 2 : 1;
        const uint32_t pw = s_w[2 + li - back];
        const bool newline = col == W - 1u, empty = w == kNoWord, first = g == 0 && lead == 0u;
        const bool staged = g + lead >= (uint64_t)back && pw != kNoWord;
        uint32_t len = colour_key<MODE>(pw) == colour_key<MODE>(w) ? 1u : kS;
        len = first ? kS : len;  // first pixel of the frame
        len = empty ? 0u : len;  // empty slot
        len = newline ? 1u : len;
        if (!newline && !empty && !first && !staged) {
            len = word_length_walk<MODE>(words, g, W, w, lead);
        }
        return len;
    }

    static __device__ __forceinline__ void emit(uint8_t* dst, uint32_t len, bool newline, uint32_t w)
    {
        if (len == kS) {
            Fields f;
            f.c0 = w & 255u;
            f.c1 = (w >> 8) & 255u;
            f.c2 = (w >> 16) & 255u;
            f.glyph = w >> 24;
            uint32_t r[kS / 4];
            record_words<MODE>(w != kCompactMiss, f, digits(), r);
#pragma unroll
            for (uint32_t q = 0; q < kS / 4u; q++) {
                *reinterpret_cast<u32_unaligned*>(dst + 4u * q) = r[q];
            }
        } else if (len == 1u) {
            // the row's newline, or the glyph alone (the last byte of the record: ' ' for a miss)
            dst[0] = newline ? (uint8_t)'\n' : (w == kCompactMiss ? (uint8_t)' ' : (uint8_t)(w >> 24));
        }
    }
};

// ---- delta frames: two frames of pixel words, `cur` and the one before it, `prev`; only the cells that changed are emitted, each
// run of them addressed by a cursor escape (rtx_delta_words in rtx.h states the rule).  No reference counterpart: its printer homes
// the cursor and rewrites the screen (PrintMachine.cpp:257-306).  Slot rules:
//   * column W-1, an empty slot (0xffffffff) of cur, cur == prev   -> nothing
//   * a changed slot whose left neighbour in the row did not change (or column 0): a run starts -> ESC [ row+1 ; col+1 H, then the
//     whole record
//   * any other changed slot -> the whole record if its first S-1 bytes differ from those of the record to its left, else its glyph
// The first S-1 bytes of a record are a function of the colour key and of the '3' / '4' selector, which differs between a hit and a
// miss in the two ASCII modes only (record_words): the head key.  Everything looks one slot back and no further, so there is no walk.
struct DeltaInput {
    const uint32_t* cur;
    const uint32_t* prev;
    unsigned long long* counts; // [0] changed cells, [1] runs of the launch, zeroed by the host
};

template <int MODE>
__device__ __forceinline__ uint32_t head_key(uint32_t w)
{
    constexpr bool kAscii = (MODE == RTX_K_BIT_ASCII || MODE == RTX_K_RGB_ASCII);
    return colour_key<MODE>(w) | ((kAscii && w != kCompactMiss) ? (1u << 24) : 0u);
}

__device__ __forceinline__ uint32_t decimal_length(uint32_t v) // v <= 99999
{
    return 1u + (v >= 10u ? 1u : 0u) + (v >= 100u ? 1u : 0u) + (v >= 1000u ? 1u : 0u) + (v >= 10000u ? 1u : 0u);
}

__device__ __forceinline__ void put_decimal(uint8_t* dst, uint32_t v, uint32_t n)
{
    for (uint32_t i = n; i-- > 0u;) {
        const uint32_t q = v / 10u;
        dst[i] = (uint8_t)(48u + (v - 10u * q));
        v = q;
    }
}

// The block's buffer, in dwords: [0] the row and [1] the column of the block's first slot, [kCur - 1] the word of cur in front of
// the block (0xffffffff where the frame begins), [kCur + li] cur of slot base + li, the same of prev from kPrev, the scan's partial
// sums behind them.  The image is built over all of it once every thread holds its own slots.
template <int MODE>
struct DeltaSource {
    typedef uint32_t Elem;
    typedef DeltaInput In;
    struct Item {
        uint32_t w, row1, col1; // the word; row + 1 and column + 1 where a run starts
    };
    static constexpr uint32_t kS = (MODE == RTX_K_RGB_ASCII || MODE == RTX_K_RGB_PIXEL || MODE == RTX_K_RGB_NORMALS) ? 20u : 12u;
    static constexpr uint32_t kCur = 4, kPrev = kCur + kSlotsPerBlock + 4;
    static constexpr uint32_t kWave = (kPrev + kSlotsPerBlock) * 4;
    static constexpr uint32_t kStage = kWave + (kThreads / 64) * 4;
    // the image: a block inside one long row -- 513 cells in 512 runs of 12-byte records, or 1024 cells of 20 bytes behind one
    // escape -- emits more than 1024 S bytes
    static constexpr uint32_t kBytes = ((uint32_t)rtxplan::delta_block_bound(kS, kSlotsPerBlock) + 15u) & ~15u;
    static_assert(kBytes >= rtxplan::delta_block_bound(kS, kSlotsPerBlock) && kBytes > kSlotsPerBlock * kS, "the image holds the longest stream a block can emit");
    static_assert(kStage <= kBytes, "words + partial sums fit the image's space");

    static In input(const void* cur, const void* prev, void* counts) { return In{(const uint32_t*)cur, (const uint32_t*)prev, (unsigned long long*)counts}; }

    static __device__ __forceinline__ uint32_t* tally()
    {
        __shared__ uint32_t s_tally[kThreads / 64];
        return s_tally;
    }

    static __device__ __forceinline__ void stage_words(const uint32_t* __restrict__ words, uint64_t base, uint64_t n_slots, uint32_t* s_w)
    {
        const uint32_t tid = threadIdx.x;
        const uint64_t g0 = base + (uint64_t)tid * kPerThread;
        if (g0 + kPerThread <= n_slots && ((uintptr_t)(words + g0) & 15u) == 0u) {
            *reinterpret_cast<uint4*>(s_w + tid * kPerThread) = *reinterpret_cast<const uint4*>(words + g0); // (kCur and kPrev are multiples of 4)
        } else {
#pragma unroll
            for (int k = 0; k < kPerThread; k++) {
                s_w[tid * kPerThread + k] = g0 + k < n_slots ? words[g0 + k] : kNoWord;
            }
        }
    }

    static __device__ __forceinline__ void stage(In in, uint64_t base, uint64_t n_slots, uint32_t, uint8_t* s, uint32_t W)
    {
        uint32_t* s_w = reinterpret_cast<uint32_t*>(s);
        stage_words(in.cur, base, n_slots, s_w + kCur);
        stage_words(in.prev, base, n_slots, s_w + kPrev);
        // the block's first row by one scalar division (64-bit only where the slot does not fit 32 bits), as first_column
        const uint32_t row0 = (uint32_t)__builtin_amdgcn_readfirstlane((base >> 32) == 0u ? (uint32_t)base / W : (uint32_t)(base / W));
        if (threadIdx.x == 0u) {
            s_w[0] = row0;
            s_w[1] = (uint32_t)(base - (uint64_t)row0 * W);
            s_w[kCur - 1] = base > 0u ? in.cur[base - 1u] : kNoWord;
            s_w[kPrev - 1] = base > 0u ? in.prev[base - 1u] : kNoWord;
        }
    }

    static __device__ __forceinline__ void stage_tables() { WordSource<MODE>::stage_tables(); }

    // Emitted length of slot g (column col, staged at li): 0, 1 (the glyph), S (the record) or S + the escape's 6 .. 14 bytes.
    static __device__ __forceinline__ uint32_t length(In, const uint8_t* s, uint64_t, int li, uint32_t col, uint32_t W, uint32_t, Item& it)
    {
        const uint32_t* s_w = reinterpret_cast<const uint32_t*>(s);
        const uint32_t w = s_w[kCur + li], left = s_w[kCur + li - 1];
        const bool changed = col != W - 1u && w != s_w[kPrev + li] && w != kNoWord;
        const bool left_changed = col != 0u && left != s_w[kPrev + li - 1] && left != kNoWord; // (column col - 1 < W - 1: a cell)
        const bool start = changed && !left_changed;
        uint32_t len = !changed ? 0u : ((start || head_key<MODE>(w) != head_key<MODE>(left)) ? kS : 1u);
        it.w = w;
        it.row1 = it.col1 = 0u;
        if (start) {
            it.row1 = s_w[0] + (s_w[1] + (uint32_t)li) / W + 1u; // (32-bit: column + 1024 < 2^31)
            it.col1 = col + 1u;
            len += 4u + decimal_length(it.row1) + decimal_length(it.col1);
        }
        return len;
    }

    static __device__ __forceinline__ void emit(uint8_t* dst, uint32_t len, bool, const Item& it)
    {
        if (len > kS) {
            const uint32_t nr = decimal_length(it.row1), nc = decimal_length(it.col1);
            dst[0] = 0x1bu;
            dst[1] = (uint8_t)'[';
            put_decimal(dst + 2, it.row1, nr);
            dst[2u + nr] = (uint8_t)';';
            put_decimal(dst + 3u + nr, it.col1, nc);
            dst[3u + nr + nc] = (uint8_t)'H';
            dst += len - kS;
            len = kS;
        }
        WordSource<MODE>::emit(dst, len, false, it.w); // the record, its glyph, or nothing
    }

    // The launch's counts: each wave's sum before a barrier of the caller's, then one atomic instruction of two lanes per block.
    static __device__ __forceinline__ void tally_put(const uint32_t* len)
    {
        uint32_t v = 0u; // changed cells | runs << 16
#pragma unroll
        for (int k = 0; k < kPerThread; k++) {
            v += (len[k] != 0u ? 1u : 0u) + (len[k] > kS ? 0x10000u : 0u);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            v += (uint32_t)__shfl_xor((int)v, d);
        }
        if ((threadIdx.x & 63u) == 0u) {
            tally()[threadIdx.x >> 6] = v;
        }
    }

    static __device__ __forceinline__ void tally_add(In in)
    {
        if (threadIdx.x < 2u) {
            uint32_t v = 0u;
#pragma unroll
            for (int k = 0; k < kThreads / 64; k++) {
                v += tally()[k];
            }
            const uint32_t mine = threadIdx.x == 0u ? (v & 0xffffu) : (v >> 16); // (at most 1024 cells and 512 runs per block)
            if (v != 0u) {
                atomicAdd(&in.counts[threadIdx.x], (unsigned long long)mine);
            }
        }
    }
};

// ---- half-block frames: W x 2H pixel words as W x H cells of U+2580, the upper half block -- the foreground colour paints pixel
// row 2r, the background colour row 2r + 1 (rtx_half_words in rtx.h states the rule).  No reference counterpart: its PIXEL modes
// paint one background colour under a space (RayTracing.cu:256,476).  Slot rules, slot g = r W + c of the W x H cells:
//   * column W-1 -> '\n'
//   * any other slot is a cell with T = key(words[2g - c]), B = key(words[2g - c + W]) (a word 0xffffffff counts as 0): the
//     foreground escape if T differs from the T of the cell before it (slot g-1, or g-2 in column 0; the frame's first cell has
//     none), the background escape likewise for B, then the glyph's three bytes.
// Every cell emits, so nothing looks further back than two slots: no walk.  RGB: the family -- r;g;b of the key's three bytes, else
// the xterm index.
//
// The block's buffer, in dwords: [kTop - 2], [kTop - 1] the top words of the two slots before the block's first, [kTop + li] the top
// word of slot base + li, the same of the bottom words from kBot, the scan's partial sums behind them.  A block's slots may span
// rows and the two words of a slot lie a row apart: slot li of row r is word base + li + r W, so consecutive lanes read consecutive
// words along each row and a row's end costs one more memory line.
template <bool RGB>
struct HalfSource {
    typedef uint32_t Elem;
    typedef const uint32_t* __restrict__ In;
    struct Item {
        uint32_t t, b; // the two keys; bit 31: the escape is due
    };
    static constexpr uint32_t kDue = 0x80000000u;
    static constexpr uint32_t kE = RGB ? (uint32_t)rtxplan::kHalfEscRgb : (uint32_t)rtxplan::kHalfEsc8;
    static constexpr uint32_t kS = 2u * kE + (uint32_t)rtxplan::kHalfGlyph; // the longest slot
    static constexpr uint32_t kTop = 4, kBot = kTop + kSlotsPerBlock + 4;
    static constexpr uint32_t kWave = (kBot + kSlotsPerBlock) * 4;
    static constexpr uint32_t kStage = kWave + (kThreads / 64) * 4;
    static constexpr uint32_t kBytes = ((uint32_t)rtxplan::half_block_bound(kE, kSlotsPerBlock) + 15u) & ~15u;
    static_assert(rtxplan::half_block_bound(kE, kSlotsPerBlock) != 0 && kBytes >= rtxplan::half_block_bound(kE, kSlotsPerBlock) && kBytes >= kSlotsPerBlock * kS,
                  "the image holds the longest stream a block can emit");
    static_assert(kStage <= kBytes, "words + partial sums fit the image's space");

    static In input(const void* data, const void*, void*) { return (In)data; }
    static __device__ __forceinline__ void stage_tables() {}
    static __device__ __forceinline__ void tally_put(const uint32_t*) {}
    static __device__ __forceinline__ void tally_add(In) {}

    static __device__ __forceinline__ uint32_t key(uint32_t w)
    {
        w = w == kNoWord ? 0u : w; // (outside column W-1, which has no key)
        return colour_key<RGB ? RTX_K_RGB_PIXEL : RTX_K_BIT_PIXEL>(w);
    }

    static __device__ __forceinline__ uint32_t digits(uint32_t v) { return 1u + (v >= 10u ? 1u : 0u) + (v >= 100u ? 1u : 0u); } // v <= 255

    static __device__ __forceinline__ uint32_t escape_length(uint32_t k)
    {
        return RGB ? 10u + digits(k & 255u) + digits((k >> 8) & 255u) + digits((k >> 16) & 255u) : 8u + digits(k);
    }

    static __device__ __forceinline__ void stage(In words, uint64_t base, uint64_t n_slots, uint32_t, uint8_t* s, uint32_t W)
    {
        uint32_t* s_w = reinterpret_cast<uint32_t*>(s);
        // the block's first row and column by one scalar division (64-bit only where the slot does not fit 32 bits), as first_column
        const uint32_t row0 = (uint32_t)__builtin_amdgcn_readfirstlane((base >> 32) == 0u ? (uint32_t)base / W : (uint32_t)(base / W));
        const uint32_t col0 = (uint32_t)(base - (uint64_t)row0 * W);
#pragma unroll
        for (int k = 0; k < kPerThread; k++) {
            const uint32_t li = (uint32_t)k * kThreads + threadIdx.x;
            uint32_t top = kNoWord, bot = kNoWord;
            if (base + li < n_slots) {
                const uint32_t row = row0 + (col0 + li) / W; // (32-bit: col0 < W < 2^31 and li < 1024)
                const uint32_t* p = words + (base + li + (uint64_t)row * W); // = words + 2g - c; the last one read is word 2 n_slots - 1
                top = p[0];
                bot = p[W];
            }
            s_w[kTop + li] = top;
            s_w[kBot + li] = bot;
        }
        if (threadIdx.x < 2u) {
            // slot base - 2 + tid: in row row0 if the block's first column is far enough right, else in the row above (whatever W:
            // a word of the frame, and one that no cell looks at where the slot is not the cell in front of it)
            const uint32_t back = 2u - threadIdx.x;
            uint32_t top = kNoWord, bot = kNoWord;
            if (base >= back) {
                const uint32_t row = col0 >= back ? row0 : row0 - 1u; // (base >= back and col0 < back: row0 >= 1)
                const uint32_t* p = words + (base - back + (uint64_t)row * W);
                top = p[0];
                bot = p[W];
            }
            s_w[kTop - back] = top;
            s_w[kBot - back] = bot;
        }
    }

    // Emitted length of slot g (column col, staged at li): 1 for the newline, else 3 plus the escapes that are due.
    static __device__ __forceinline__ uint32_t length(In, const uint8_t* s, uint64_t g, int li, uint32_t col, uint32_t W, uint32_t, Item& it)
    {
        const uint32_t* s_w = reinterpret_cast<const uint32_t*>(s);
        const int back = col == 0u ? 2 : 1; // the cell before: slot g-1, or g-2 when g-1 is the row above's last column
        const uint32_t t = key(s_w[kTop + li]), b = key(s_w[kBot + li]);
        const uint32_t pt = key(s_w[(int)kTop + li - back]), pb = key(s_w[(int)kBot + li - back]);
        const bool first = g == 0u, newline = col == W - 1u;
        const bool due_t = first || t != pt, due_b = first || b != pb;
        it.t = t | (due_t ? kDue : 0u);
        it.b = b | (due_b ? kDue : 0u);
        const uint32_t len = (uint32_t)rtxplan::kHalfGlyph + (due_t ? escape_length(t) : 0u) + (due_b ? escape_length(b) : 0u);
        return newline ? 1u : len;
    }

    // ESC [ sel 8 ; 2 ; r ; g ; b m  resp.  ESC [ sel 8 ; 5 ; K m  at dst; returns its length.  The head goes out as two dwords: the
    // eighth byte is the first digit's place, which is written afterwards (32-bit stores into LDS need no alignment).
    static __device__ __forceinline__ uint32_t put_escape(uint8_t* dst, uint32_t sel, uint32_t k)
    {
        *reinterpret_cast<u32_unaligned*>(dst) = 0x1bu | ((uint32_t)'[' << 8) | (sel << 16) | ((uint32_t)'8' << 24);
        *reinterpret_cast<u32_unaligned*>(dst + 4) = (uint32_t)';' | ((RGB ? (uint32_t)'2' : (uint32_t)'5') << 8) | ((uint32_t)';' << 16) | ((uint32_t)'0' << 24);
        uint32_t at = 7u;
#pragma unroll
        for (uint32_t q = 0; q < (RGB ? 3u : 1u); q++) {
            const uint32_t v = (k >> (8u * q)) & 255u, n = digits(v);
            put_decimal(dst + at, v, n);
            dst[at + n] = q + 1u < (RGB ? 3u : 1u) ? (uint8_t)';' : (uint8_t)'m';
            at += n + 1u;
        }
        return at;
    }

    static __device__ __forceinline__ void emit(uint8_t* dst, uint32_t len, bool newline, const Item& it)
    {
        if (len == 0u) {
            return; // a slot past the frame's end
        }
        if (newline) {
            dst[0] = (uint8_t)'\n';
            return;
        }
        if ((it.t & kDue) != 0u) dst += put_escape(dst, (uint32_t)'3', it.t & ~kDue);
        if ((it.b & kDue) != 0u) dst += put_escape(dst, (uint32_t)'4', it.b & ~kDue);
        dst[0] = 0xe2u;
        dst[1] = 0x96u;
        dst[2] = 0x80u;
    }
};

// ---- delta frames of half-block streams: two frames of W x 2H pixel words, `cur` and the one before it, `prev`; only the cells whose
// (T, B) keys changed are emitted, each run of them addressed by a cursor escape (rtx_half_delta_words in rtx.h states the rule).  No
// reference counterpart (RayTracing.cu:256,476; PrintMachine.cpp:257-306).  Slot rules, slot g = r W + c of the W x H cells:
//   * column W-1, a cell whose keys (T, B) are those of prev                -> nothing
//   * a changed cell whose left neighbour in the row did not change (or column 0): a run starts -> ESC [ row+1 ; col+1 H, then
//     both colour escapes (whatever the terminal's colours were: a run relies on nothing before it) and the glyph
//   * any other changed cell -> the foreground escape if T differs from the T of the cell to its left in cur, the background escape
//     likewise for B, then the glyph
// Column 0 always starts a run, so a cell looks at slot g-1 of its own row and no further: one slot of halo, no walk.
//
// The block's buffer, in dwords: [0] the row and [1] the column of the block's first slot; four arrays of the block's slots, each
// with the slot in front of the block at [k - 1] (0xffffffff where that slot is not in the block's first row: nothing looks at
// it then) -- top and bottom words of cur from kCurTop and kCurBot, of prev from kPrevTop and kPrevBot -- and the scan's partial
// sums behind them.  Words are addressed as HalfSource::stage addresses them: consecutive lanes read consecutive words along each
// row.  The image is built over all of it once every thread holds its own slots.
template <bool RGB>
struct HalfDeltaSource {
    typedef HalfSource<RGB> Half;
    typedef uint32_t Elem;
    typedef DeltaInput In;
    struct Item {
        uint32_t t, b;       // the two keys; bit 31: the escape is due
        uint32_t row1, col1; // row + 1 and column + 1 where a run starts, else 0: a start cannot be told from a length (35 .. 55
                             // bytes in the RGB family against 3 .. 41 of a cell inside a run)
    };
    static constexpr uint32_t kDue = Half::kDue;
    static constexpr uint32_t kE = Half::kE;
    static constexpr uint32_t kS = Half::kS; // the longest cell inside a run
    static constexpr uint32_t kCurTop = 4, kCurBot = kCurTop + kSlotsPerBlock + 4, kPrevTop = kCurBot + kSlotsPerBlock + 4, kPrevBot = kPrevTop + kSlotsPerBlock + 4;
    static constexpr uint32_t kWave = (kPrevBot + kSlotsPerBlock) * 4;
    static constexpr uint32_t kStage = kWave + (kThreads / 64) * 4;
    // the image: 1024 cells of 2E + 3 bytes behind one escape when a run starts on the block's first slot
    static constexpr uint32_t kBytes = ((uint32_t)rtxplan::half_delta_block_bound(kE, kSlotsPerBlock) + 15u) & ~15u;
    static_assert(rtxplan::half_delta_block_bound(kE, kSlotsPerBlock) != 0 && kBytes >= rtxplan::half_delta_block_bound(kE, kSlotsPerBlock) &&
                      kBytes > kSlotsPerBlock * kS,
                  "the image holds the longest stream a block can emit");
    static_assert(kStage <= kBytes, "words + partial sums fit the image's space");

    static In input(const void* cur, const void* prev, void* counts) { return In{(const uint32_t*)cur, (const uint32_t*)prev, (unsigned long long*)counts}; }
    static __device__ __forceinline__ void stage_tables() {}

    // changed cells | runs << 16 of each wave: the cells from the lengths (tally_put), the runs from the items as they are emitted
    static __device__ __forceinline__ uint32_t* tally()
    {
        __shared__ uint32_t s_tally[kThreads / 64];
        return s_tally;
    }

    static __device__ __forceinline__ void stage(In in, uint64_t base, uint64_t n_slots, uint32_t, uint8_t* s, uint32_t W)
    {
        uint32_t* s_w = reinterpret_cast<uint32_t*>(s);
        // the block's first row and column by one scalar division (64-bit only where the slot does not fit 32 bits), as first_column
        const uint32_t row0 = (uint32_t)__builtin_amdgcn_readfirstlane((base >> 32) == 0u ? (uint32_t)base / W : (uint32_t)(base / W));
        const uint32_t col0 = (uint32_t)(base - (uint64_t)row0 * W);
#pragma unroll
        for (int k = 0; k < kPerThread; k++) {
            const uint32_t li = (uint32_t)k * kThreads + threadIdx.x;
            uint32_t ct = kNoWord, cb = kNoWord, pt = kNoWord, pb = kNoWord;
            if (base + li < n_slots) {
                const uint32_t row = row0 + (col0 + li) / W; // (32-bit: col0 < W <= 100000 and li < 1024)
                const uint64_t at = base + li + (uint64_t)row * W; // = 2g - c; the last word read is word 2 n_slots - 1
                ct = in.cur[at];
                cb = in.cur[at + W];
                pt = in.prev[at];
                pb = in.prev[at + W];
            }
            s_w[kCurTop + li] = ct;
            s_w[kCurBot + li] = cb;
            s_w[kPrevTop + li] = pt;
            s_w[kPrevBot + li] = pb;
        }
        if (threadIdx.x == 0u) {
            uint32_t ct = kNoWord, cb = kNoWord, pt = kNoWord, pb = kNoWord;
            if (col0 >= 1u) { // slot base - 1 is the cell to the left of the block's first, in row row0 (base >= col0 >= 1)
                const uint64_t at = base - 1u + (uint64_t)row0 * W;
                ct = in.cur[at];
                cb = in.cur[at + W];
                pt = in.prev[at];
                pb = in.prev[at + W];
            }
            s_w[0] = row0;
            s_w[1] = col0;
            s_w[kCurTop - 1] = ct;
            s_w[kCurBot - 1] = cb;
            s_w[kPrevTop - 1] = pt;
            s_w[kPrevBot - 1] = pb;
        }
        if (threadIdx.x < (uint32_t)(kThreads / 64)) {
            tally()[threadIdx.x] = 0u;
        }
    }

    // Emitted length of slot g (column col, staged at li): 0, or 3 plus the escapes that are due plus, where a run starts, the
    // cursor escape's 6 .. 14 bytes.
    static __device__ __forceinline__ uint32_t length(In, const uint8_t* s, uint64_t, int li, uint32_t col, uint32_t W, uint32_t, Item& it)
    {
        const uint32_t* s_w = reinterpret_cast<const uint32_t*>(s);
        const uint32_t t = Half::key(s_w[(int)kCurTop + li]), b = Half::key(s_w[(int)kCurBot + li]);
        const uint32_t lt = Half::key(s_w[(int)kCurTop + li - 1]), lb = Half::key(s_w[(int)kCurBot + li - 1]); // (staged whatever li: the halo)
        const bool changed = col != W - 1u && (t != Half::key(s_w[(int)kPrevTop + li]) || b != Half::key(s_w[(int)kPrevBot + li]));
        const bool left_changed = col != 0u && (lt != Half::key(s_w[(int)kPrevTop + li - 1]) || lb != Half::key(s_w[(int)kPrevBot + li - 1])); // (column col - 1 < W - 1: a cell)
        const bool start = changed && !left_changed;
        const bool due_t = start || t != lt, due_b = start || b != lb;
        it.t = t | (due_t ? kDue : 0u);
        it.b = b | (due_b ? kDue : 0u);
        it.row1 = it.col1 = 0u;
        uint32_t len = (uint32_t)rtxplan::kHalfGlyph + (due_t ? Half::escape_length(t) : 0u) + (due_b ? Half::escape_length(b) : 0u);
        if (start) {
            it.row1 = s_w[0] + (s_w[1] + (uint32_t)li) / W + 1u; // (32-bit: column + 1024 < 2^31)
            it.col1 = col + 1u;
            len += 4u + decimal_length(it.row1) + decimal_length(it.col1);
        }
        return changed ? len : 0u;
    }

    static __device__ __forceinline__ void emit(uint8_t* dst, uint32_t len, bool, const Item& it)
    {
        if (len == 0u) {
            return; // an unchanged cell, a row's last column, a slot past the frame's end
        }
        if (it.row1 != 0u) {
            const uint32_t nr = decimal_length(it.row1), nc = decimal_length(it.col1);
            dst[0] = 0x1bu;
            dst[1] = (uint8_t)'[';
            put_decimal(dst + 2, it.row1, nr);
            dst[2u + nr] = (uint8_t)';';
            put_decimal(dst + 3u + nr, it.col1, nc);
            dst[3u + nr + nc] = (uint8_t)'H';
            dst += 4u + nr + nc;
            atomicAdd(&tally()[threadIdx.x >> 6], 0x10000u); // a run of the launch (LDS, no return value; zeroed by stage())
        }
        if ((it.t & kDue) != 0u) dst += Half::put_escape(dst, (uint32_t)'3', it.t & ~kDue);
        if ((it.b & kDue) != 0u) dst += Half::put_escape(dst, (uint32_t)'4', it.b & ~kDue);
        dst[0] = 0xe2u;
        dst[1] = 0x96u;
        dst[2] = 0x80u;
    }

    // The launch's counts, as DeltaSource's: each wave's sum before a barrier of the caller's, then one atomic instruction of two
    // lanes per block.  The lengths give the changed cells; the runs were counted as their escapes were written (emit).
    static __device__ __forceinline__ void tally_put(const uint32_t* len)
    {
        uint32_t v = 0u;
#pragma unroll
        for (int k = 0; k < kPerThread; k++) {
            v += len[k] != 0u ? 1u : 0u;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            v += (uint32_t)__shfl_xor((int)v, d);
        }
        if ((threadIdx.x & 63u) == 0u && v != 0u) {
            atomicAdd(&tally()[threadIdx.x >> 6], v);
        }
    }

    static __device__ __forceinline__ void tally_add(In in)
    {
        if (threadIdx.x < 2u) {
            uint32_t v = 0u;
#pragma unroll
            for (int k = 0; k < kThreads / 64; k++) {
                v += tally()[k];
            }
            const uint32_t mine = threadIdx.x == 0u ? (v & 0xffffu) : (v >> 16); // (at most 1024 cells and 512 runs per block)
            if (v != 0u) {
                atomicAdd(&in.counts[threadIdx.x], (unsigned long long)mine);
            }
        }
    }
};

// ---- the chain: rtx_min_count -> rtx_min_offsets -> rtx_min_scatter, three launches.
// The blocks' sums -> their offsets in the stream (exclusive scan; one workgroup, 2048 sums per step) and the stream's length.
// A launch of its own between the two passes: the scatter pass then finds its place with one load, where summing the preceding
// blocks' sums in every block cost a chain of dependent L2 round trips per block and O(blocks^2) loads per frame (32 400 blocks
// at 8K).  (Letting the count pass's last block do this -- a ticket drawn with atomicAdd -- was measured: 2025 device-scope
// atomics on one address take 46 us, 22 ns each.)
__global__ __launch_bounds__(kThreads) void rtx_min_offsets(const uint32_t* __restrict__ block_sums, uint32_t nb, uint64_t* __restrict__ offsets, uint64_t* total_out)
{
    __shared__ uint32_t s_wave[kThreads / 64];
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += 8u * kThreads) {
        uint32_t v[8], mine = 0;
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) {
            const uint32_t i = b0 + threadIdx.x * 8u + q;
            v[q] = i < nb ? block_sums[i] : 0u;
            mine += v[q];
        }
        uint32_t step_total;
        uint64_t at = carry + block_exclusive_scan(mine, s_wave, step_total);
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) {
            const uint32_t i = b0 + threadIdx.x * 8u + q;
            if (i < nb) offsets[i] = at;
            at += v[q];
        }
        carry += step_total;
    }
    if (threadIdx.x == 0) {
        *total_out = carry; // length of the minimised stream
    }
}

// ---- the same pass as ONE launch (rtx_min_fused): count, offsets and scatter of the chain in one kernel, the block offsets by a
// two-level look-back.  Three dependent launches of a few microseconds each pay two launch gaps and read the input twice; here a
// block counts its slots, publishes its length, builds its output bytes in LDS while the other blocks do the same, and then finds
// where its bytes go:
//   * agg[b]  = (epoch << 32) | length of block b            published by every block as soon as it has counted
//   * grp[r][g] = (epoch << 32) | length of blocks 64g..64g+63  published by the LAST block of the group, which reads the other 63
//     lengths for its own offset anyway; 64 replicas r (rows of `ng` entries), block b reads replica b % 64
//   * offset of block b = sum of grp[b % 64][0 .. b/64) + sum of agg[64 (b/64) .. b): one wave, one or a few loads per lane, two
//     dependent steps for every block however many blocks there are (no chain of prefixes from block to block).
// A block waits only for blocks with smaller indices; workgroups are dispatched in index order on every XCD, so the unfinished
// block with the smallest index never waits and the launch drains.  All the same nothing here spins without a bound: a lane that
// has polled max_polls times gives up, the block writes the launch's epoch into the failure word and stores nothing, a group's
// last block that gave up publishes a poisoned total (the later blocks then give up at once), and the host runs the chain
// instead (launch_minimize, settle_minimize).  Entries carry the launch's epoch, so the tables are never cleared between
// launches; they are zeroed when allocated and epoch 0 is never used.
constexpr uint32_t kLookGroup = 64u;
constexpr uint32_t kLookPoison = 0xffffffffu;
constexpr uint32_t kLookPolls = 1u << 18; // x >= 0.5 us per poll: at least a tenth of a second

__device__ __forceinline__ bool look_wait(const uint64_t* p, uint32_t epoch, uint32_t max_polls, uint32_t& value)
{
    for (uint32_t i = 0;; i++) {
        const uint64_t e = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint32_t)(e >> 32) == epoch) {
            value = (uint32_t)e;
            return true;
        }
        if (i >= max_polls) {
            value = 0u;
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// The look-back of block b, whose length n is already published in agg[b]: done by the first wave, the block's offset in *s_G and
// the verdict in *s_ok (both in LDS), a barrier, and the verdict returned to every thread.  The barrier also completes whatever the
// block wrote to LDS before the call (its output image).
__device__ __forceinline__ bool look_back(uint32_t b, uint32_t n, const uint64_t* agg, uint64_t* grp, uint32_t ng, uint32_t epoch, uint32_t max_polls, uint64_t* s_G,
                                          uint32_t* s_ok)
{
    if (threadIdx.x < 64u) {
        const uint32_t lane = threadIdx.x;
        const uint32_t g = b / kLookGroup, first = g * kLookGroup;
        uint64_t before = 0, in_group = 0;
        bool ok_group = true, ok_before = true;
        if (first + lane < b) {
            uint32_t v;
            ok_group = look_wait(&agg[first + lane], epoch, max_polls, v);
            in_group = v;
        }
        if (max_polls == 0u && b % 3u == 1u) {
            ok_group = false; // (tests: a launch whose blocks give up, RTX_OPT_MINIMIZE_FUSED = 2)
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            in_group += __shfl_xor(in_group, d);
        }
        ok_group = __all(ok_group);
        if (b % kLookGroup == kLookGroup - 1u) {
            // the group's total, once per replica (lane r writes replica r: 64 lines) and BEFORE this block looks at the totals
            // of the groups before it: a total depends on its own group only, so all of them appear at about the same time
            // (published after that look, they formed a chain, 0.85 us per group: 30 us at 1080p)
            const uint32_t t = ok_group ? (uint32_t)in_group + n : kLookPoison;
            __hip_atomic_store(&grp[(size_t)lane * ng + g], ((uint64_t)epoch << 32) | t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // (replica b % 64 of the totals, so that a total's readers are spread over 64 lines)
        const uint64_t* my_grp = grp + (size_t)(b % kLookGroup) * ng;
        for (uint32_t q = lane; q < g && ok_before; q += 64u) {
            uint32_t v;
            ok_before = look_wait(&my_grp[q], epoch, max_polls, v) && v != kLookPoison;
            before += v;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            before += __shfl_xor(before, d);
        }
        ok_before = __all(ok_before);
        if (lane == 0u) {
            *s_G = before + in_group;
            *s_ok = (ok_group && ok_before) ? 1u : 0u;
        }
    }
    __syncthreads();
    return *s_ok != 0u;
}

// The block's image, bytes [at, at + n) of the LDS buffer `s` (16-byte aligned), to out[G, G + n).  Head and tail of partial 16-byte
// lines of the destination go out byte by byte, the lines between as uint4: read as such when the image has G's 16-byte phase
// (at = G & 15: the scatter pass knows G before it builds the image), else -- an image at offset 0 whatever G's phase: the one-launch
// form learns G only afterwards -- as five aligned dwords and a byte shift per line (four unaligned dword reads become an unaligned
// ds_read_b128, which is slow: the one-launch form ran 45 us with them).
__device__ __forceinline__ void copy_out_image(const uint8_t* s, uint32_t at, uint32_t n, uint64_t G, uint8_t* out)
{
    const uint32_t pad = (uint32_t)(G & 15u);
    const uint32_t head = n < ((16u - pad) & 15u) ? n : ((16u - pad) & 15u);
    const uint32_t body16 = (n - head) / 16u;
    const uint32_t tail = n - head - body16 * 16u;
    if (threadIdx.x < head) {
        out[G + threadIdx.x] = s[at + threadIdx.x];
    }
    const uint32_t b0 = at + head; // LDS byte of the first whole line
    uint4* dst16 = reinterpret_cast<uint4*>(out + G + head);
    if ((b0 & 15u) == 0u) {
        const uint4* src = reinterpret_cast<const uint4*>(s + b0);
        for (uint32_t i = threadIdx.x; i < body16; i += kThreads) {
            dst16[i] = src[i];
        }
    } else {
        const uint32_t* src32 = reinterpret_cast<const uint32_t*>(s + (b0 & ~3u));
        const uint32_t shift = b0 & 3u;
        for (uint32_t i = threadIdx.x; i < body16; i += kThreads) {
            // (the fifth dword of the image's last line may lie past the image: read only what exists)
            const uint32_t a0 = src32[4u * i], a1 = src32[4u * i + 1u], a2 = src32[4u * i + 2u], a3 = src32[4u * i + 3u];
            const uint32_t a4 = shift != 0u ? src32[4u * i + 4u] : 0u;
            uint4 v;
            v.x = __builtin_amdgcn_alignbyte(a1, a0, shift);
            v.y = __builtin_amdgcn_alignbyte(a2, a1, shift);
            v.z = __builtin_amdgcn_alignbyte(a3, a2, shift);
            v.w = __builtin_amdgcn_alignbyte(a4, a3, shift);
            dst16[i] = v;
        }
    }
    if (threadIdx.x < tail) {
        out[G + head + body16 * 16u + threadIdx.x] = s[b0 + body16 * 16u + threadIdx.x];
    }
}

// ---- the block body of the three kernels: stage the block's slots, four lengths per thread and their block-wide scan
// (min_lengths); then the block's output bytes as an LDS image (min_image), which copy_out_image writes out.
template <class Src>
struct MinBlock {
    uint32_t len[kPerThread];
    bool newline[kPerThread]; // the slot is its row's last column
    typename Src::Item item[kPerThread];
    uint32_t at, n; // this thread's first byte in the block's image; the block's length
};

// kImage: the block's image follows, which needs each thread's four slots consecutive; else (a count: only the sum matters) slot
// k of thread t is k * kThreads + t, so that consecutive lanes read consecutive slots (bank-conflict free at the records' stride).
template <class Src, bool kImage>
__device__ __forceinline__ void min_lengths(typename Src::In in, uint64_t n_slots, uint32_t W, uint32_t lead, uint8_t* s, MinBlock<Src>& m)
{
    const uint64_t base = (uint64_t)blockIdx.x * kSlotsPerBlock;
    Src::stage(in, base, n_slots, lead, s, W);
    if (kImage) {
        Src::stage_tables();
    }
    const int li0 = kImage ? (int)threadIdx.x * kPerThread : (int)threadIdx.x, step = kImage ? 1 : kThreads;
    const uint32_t col_step = kImage ? 1u : (uint32_t)kThreads % W;
    uint32_t col = first_column(base, W, (uint32_t)li0);
    __syncthreads();
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; k++) {
        const int li = li0 + k * step;
        const uint64_t g = base + (uint64_t)li;
        m.len[k] = 0u;
        m.newline[k] = col == W - 1u;
        if (g < n_slots) {
            m.len[k] = Src::length(in, s, g, li, col, W, lead, m.item[k]);
        }
        mine += m.len[k];
        col += col_step;
        col = col >= W ? col - W : col;
    }
    // (the scan's barriers: every thread has read its slots, the LDS in front of kWave is free for the image)
    m.at = block_exclusive_scan(mine, reinterpret_cast<uint32_t*>(s + Src::kWave), m.n);
}

template <class Src>
__device__ __forceinline__ void min_image(const MinBlock<Src>& m, uint8_t* s)
{
    uint32_t at = m.at;
#pragma unroll
    for (int k = 0; k < kPerThread; k++) {
        Src::emit(s + at, m.len[k], m.newline[k], m.item[k]);
        at += m.len[k];
    }
}

template <class Src>
__global__ __launch_bounds__(kThreads) void rtx_min_count(typename Src::In in, uint64_t n_slots, uint32_t W, uint32_t lead, uint32_t* block_sums)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_buf[Src::kStage];
    MinBlock<Src> m;
    min_lengths<Src, false>(in, n_slots, W, lead, s_buf, m);
    if (threadIdx.x == 0) {
        block_sums[blockIdx.x] = m.n;
    }
}

template <class Src>
__global__ __launch_bounds__(kThreads) void rtx_min_scatter(typename Src::In in, uint64_t n_slots, uint32_t W, uint32_t lead,
                                                            const uint64_t* __restrict__ offsets, uint8_t* out)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_buf[16 + Src::kBytes]; // (the image starts at G's 16-byte phase)
    const uint64_t G = offsets[blockIdx.x]; // where this block's output starts
    MinBlock<Src> m;
    min_lengths<Src, true>(in, n_slots, W, lead, s_buf, m);
    const uint32_t pad = (uint32_t)(G & 15u);
    min_image(m, s_buf + pad);
    Src::tally_put(m.len);
    __syncthreads();
    Src::tally_add(in);
    copy_out_image(s_buf, pad, m.n, G, out);
}

template <class Src>
__global__ __launch_bounds__(kThreads) void rtx_min_fused(typename Src::In in, uint64_t n_slots, uint32_t W, uint32_t lead, uint64_t* agg,
                                                          uint64_t* grp, uint32_t ng, uint32_t epoch, uint32_t max_polls, uint8_t* out, uint64_t* total_out)
{
    // (What bounds this launch is the order its dependency imposes on the whole GPU -- every block reads and counts, then every
    // block waits two memory round trips, then every block writes: per-block time stamps of a 1080p frame show lengths published at
    // 2-4 us, offsets known at 6-8, the last byte written at 12.7 -- not the number of resident blocks or of instructions: a build
    // with 20 480 bytes of LDS, eight blocks per CU and all 2025 blocks in one dispatch round was no faster, nor was halving the
    // instructions of the length pass.  EXPERIMENTS.md R4.5.)
    __shared__ __attribute__((aligned(16))) uint8_t s_buf[Src::kBytes];
    __shared__ uint64_t s_G;
    __shared__ uint32_t s_ok;
    const uint32_t b = blockIdx.x;
    MinBlock<Src> m;
    min_lengths<Src, true>(in, n_slots, W, lead, s_buf, m);
    if (threadIdx.x == 0) {
        __hip_atomic_store(&agg[b], ((uint64_t)epoch << 32) | m.n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    min_image(m, s_buf); // the output bytes, built while the other blocks publish their lengths
    Src::tally_put(m.len); // (a delta source's counts; the look-back's barrier stands between the two halves)
    if (!look_back(b, m.n, agg, grp, ng, epoch, max_polls, &s_G, &s_ok)) {
        if (threadIdx.x == 0) {
            total_out[1] = epoch; // the host runs the chain over the same input
        }
        return;
    }
    Src::tally_add(in);
    copy_out_image(s_buf, 0u, m.n, s_G, out);
    if (b == gridDim.x - 1u && threadIdx.x == 0) {
        total_out[0] = s_G + m.n; // length of the minimised stream
    }
}

} // namespace rtx
