// The owning types of csrc/rtx_mem.hpp without a GPU and without a HIP library: the HIP entry points the header calls are defined
// here, backed by malloc, with a log of calls, a count of live objects and a switch that makes the k-th allocation fail.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_mem.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

std::vector<std::string> g_log;
long g_live = 0;       // device + pinned blocks, events and streams alive
long g_alloc_calls = 0;
long g_fail_at = 0;    // not 0: the allocation call with this number fails
hipError_t g_last = hipSuccess;
void* g_last_freed = nullptr;

hipError_t allocate(const char* what, void** p, size_t bytes)
{
    g_log.push_back(std::string(what) + " " + std::to_string(bytes));
    if (++g_alloc_calls == g_fail_at) {
        *p = nullptr;
        g_last = hipErrorOutOfMemory;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    g_live++;
    return hipSuccess;
}

hipError_t release(const char* what, void* p)
{
    g_log.push_back(what);
    g_last_freed = p;
    std::free(p);
    g_live--;
    return hipSuccess;
}

int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            g_failed++;                                                      \
        }                                                                    \
    } while (0)

bool log_is(std::initializer_list<const char*> want)
{
    std::vector<std::string> w(want.begin(), want.end());
    const bool same = w == g_log;
    if (!same) {
        std::printf("  the log:");
        for (const auto& e : g_log) std::printf(" [%s]", e.c_str());
        std::printf("\n");
    }
    g_log.clear();
    return same;
}

} // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return allocate("hipMalloc", p, bytes); }
hipError_t hipFree(void* p) { return release("hipFree", p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) { return allocate(flags == hipHostMallocDefault ? "hipHostMalloc" : "hipHostMalloc(flags)", p, bytes); }
hipError_t hipHostFree(void* p) { return release("hipHostFree", p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags)
{
    return allocate(flags == hipEventDisableTiming ? "hipEventCreateWithFlags(no timing)" : "hipEventCreateWithFlags(timing)", (void**)e, 0);
}
hipError_t hipEventDestroy(hipEvent_t e) { return release("hipEventDestroy", e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags)
{
    return allocate(flags == hipStreamNonBlocking ? "hipStreamCreateWithFlags(non-blocking)" : "hipStreamCreateWithFlags", (void**)s, 0);
}
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return allocate("hipStreamCreateWithPriority", (void**)s, 0); }
hipError_t hipStreamDestroy(hipStream_t s) { return release("hipStreamDestroy", s); }
hipError_t hipStreamSynchronize(hipStream_t s)
{
    g_log.push_back(s ? "hipStreamSynchronize(s)" : "hipStreamSynchronize(0)");
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void)
{
    g_log.push_back("hipDeviceSynchronize");
    return hipSuccess;
}
hipError_t g_copy_result = hipSuccess; // what the next copies to the host return
hipError_t hipSetDevice(int device)
{
    g_log.push_back("hipSetDevice " + std::to_string(device));
    return hipSuccess;
}
hipError_t hipMemcpy(void* to, const void* from, size_t bytes, hipMemcpyKind kind)
{
    g_log.push_back(std::string(kind == hipMemcpyDeviceToHost ? "hipMemcpy(to host) " : "hipMemcpy ") + std::to_string(bytes));
    if (g_copy_result == hipSuccess) std::memcpy(to, from, bytes);
    return g_copy_result;
}
hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t s)
{
    g_log.push_back(std::string(s ? "hipMemsetAsync(s) " : "hipMemsetAsync(0) ") + std::to_string(bytes));
    std::memset(p, v, bytes);
    return hipSuccess;
}
hipError_t hipGetLastError(void)
{
    const hipError_t e = g_last;
    g_last = hipSuccess;
    return e;
}
}

using namespace rtxmem;

namespace {

// what the context's per-stream sets look like: buffers and events inside a struct inside a vector
struct Set {
    int tag = 0;
    DeviceBuf<uint32_t> a, b;
    PinnedBuf<float> h;
    Event ev;
};

void test_reserve()
{
    hipStream_t s = (hipStream_t)(uintptr_t)0x10; // (a handle the fakes only compare with null)
    {
        DeviceBuf<uint32_t> b;
        CHECK(b.get() == nullptr && b.capacity() == 0);
        CHECK(b.reserve(0, after_device()) == hipSuccess && log_is({})); // nothing asked for: no call
        CHECK(b.reserve(100, after_device()) == hipSuccess);
        CHECK(log_is({"hipMalloc 400"})); // (nothing to wait for, nothing to free)
        CHECK(b.get() != nullptr && b.capacity() == 100 && g_live == 1);
        uint32_t* first = b.get();
        CHECK(b.reserve(100, after_device()) == hipSuccess && b.reserve(7, after_stream(s)) == hipSuccess && b.reserve(0, nothing()) == hipSuccess);
        CHECK(log_is({}) && b.get() == first); // within the capacity: no call at all
        CHECK(b.reserve(101, nothing()) == hipSuccess);
        CHECK(log_is({"hipFree", "hipMalloc 404"}) && g_last_freed == first && b.capacity() == 101); // exactly what was asked for
        CHECK(b.reserve(200, after_stream(s)) == hipSuccess);
        CHECK(log_is({"hipStreamSynchronize(s)", "hipFree", "hipMalloc 800"}));
        CHECK(b.reserve(300, after_device()) == hipSuccess);
        CHECK(log_is({"hipDeviceSynchronize", "hipFree", "hipMalloc 1200"}));
        b.get()[299] = 1u; // (the sanitizer sees the whole capacity)
        b.release();
        CHECK(log_is({"hipFree"}) && b.get() == nullptr && b.capacity() == 0 && g_live == 0);
        b.release();
        CHECK(log_is({}));
        CHECK(b.reserve(5, after_device()) == hipSuccess && log_is({"hipMalloc 20"}));
    }
    CHECK(log_is({"hipFree"}) && g_live == 0);
    {
        PinnedBuf<uint64_t> h;
        CHECK(h.reserve(2, nothing()) == hipSuccess && log_is({"hipHostMalloc 16"}));
        CHECK(h.reserve(2, nothing()) == hipSuccess && log_is({}));
        h.get()[1] = 7;
        PinnedBuf<volatile uint32_t> v; // (the feedback words the device writes under the host's eyes)
        CHECK(v.reserve(1, nothing()) == hipSuccess && log_is({"hipHostMalloc 4"}));
        *v.get() = 3u;
        CHECK(*v.get() == 3u);
    }
    CHECK(log_is({"hipHostFree", "hipHostFree"}) && g_live == 0);
}

void test_doubling()
{
    {
        // the scene store and rtx_sort_scene: 1024, 2048, ...
        DeviceBuf<uint32_t> b;
        CHECK(b.reserve_doubling(1, 1024, nothing()) == hipSuccess && b.capacity() == 1024);
        CHECK(b.reserve_doubling(1024, 1024, nothing()) == hipSuccess && b.capacity() == 1024);
        CHECK(log_is({"hipMalloc 4096"}));
        CHECK(b.reserve_doubling(1025, 1024, after_device()) == hipSuccess && b.capacity() == 2048);
        CHECK(log_is({"hipDeviceSynchronize", "hipFree", "hipMalloc 8192"}));
        CHECK(b.reserve_doubling(5000, 1024, nothing()) == hipSuccess && b.capacity() == 8192);
        DeviceBuf<uint32_t> c;
        CHECK(c.reserve_doubling(300000, 1024, nothing()) == hipSuccess && c.capacity() == 524288); // the first power-of-two multiple that holds it
        // the edit rows: seven floats a row, from 7 * 1024
        DeviceBuf<float> rows;
        CHECK(rows.reserve_doubling(7 * 300, 7 * 1024, nothing()) == hipSuccess && rows.capacity() == 7168);
        CHECK(rows.reserve_doubling(7 * 1025, 7 * 1024, nothing()) == hipSuccess && rows.capacity() == 14336);
        CHECK(rows.reserve_doubling(7 * 5000, 7 * 1024, nothing()) == hipSuccess && rows.capacity() == 57344);
        // the removal marks (pinned bytes, from 4096) and the look-back tables (two words per block, blocks from 4096)
        PinnedBuf<uint8_t> marks;
        CHECK(marks.reserve_doubling(302, 4096, nothing()) == hipSuccess && marks.capacity() == 4096);
        CHECK(marks.reserve_doubling(4097, 4096, nothing()) == hipSuccess && marks.capacity() == 8192);
        DeviceBuf<uint64_t> look;
        CHECK(look.reserve_doubling(2 * 1, 2 * 4096, nothing()) == hipSuccess && look.capacity() / 2 == 4096);
        CHECK(look.reserve_doubling(2 * 4097, 2 * 4096, nothing()) == hipSuccess && look.capacity() / 2 == 8192);
        g_log.clear();
    }
    CHECK(g_live == 0);
    g_log.clear();
}

void test_failed_grow()
{
    {
        DeviceBuf<uint32_t> b;
        CHECK(b.reserve(10, nothing()) == hipSuccess);
        g_log.clear();
        g_fail_at = g_alloc_calls + 1;
        CHECK(b.reserve(20, after_device()) == hipErrorOutOfMemory);
        CHECK(log_is({"hipDeviceSynchronize", "hipFree", "hipMalloc 80"}));
        CHECK(b.get() == nullptr && b.capacity() == 0 && g_live == 0); // empty, as every grow block left it
        CHECK(g_last == hipSuccess);                                   // the sticky error is gone: a later launch check reports its own
        CHECK(b.reserve(20, after_device()) == hipSuccess && b.capacity() == 20);
        CHECK(log_is({"hipMalloc 80"}));
        g_fail_at = g_alloc_calls + 1;
        CHECK(b.reserve_doubling(21, 1024, nothing()) == hipErrorOutOfMemory && b.capacity() == 0 && g_last == hipSuccess);
        CHECK(b.reserve_doubling(21, 1024, nothing()) == hipSuccess && b.capacity() == 1024);
        PinnedBuf<uint32_t> h;
        g_fail_at = g_alloc_calls + 1;
        CHECK(h.reserve(1, nothing()) == hipErrorOutOfMemory && h.get() == nullptr && g_last == hipSuccess);
        CHECK(h.reserve(1, nothing()) == hipSuccess);
        // a set half built when memory runs out goes with its scope (tile_order_set)
        Set fresh;
        g_fail_at = g_alloc_calls + 3;
        const bool ok = fresh.a.reserve(8, nothing()) == hipSuccess && fresh.b.reserve(8, nothing()) == hipSuccess && fresh.h.reserve(8, nothing()) == hipSuccess &&
                        fresh.ev.ensure() == hipSuccess;
        CHECK(!ok && fresh.a.get() && fresh.b.get() && !fresh.h.get() && !fresh.ev.get());
        g_fail_at = 0;
    }
    CHECK(g_live == 0);
    g_log.clear();
}

void test_moves()
{
    {
        std::vector<Set> v; // (no reserve: the vector reallocates as it grows, moving every set)
        for (int i = 0; i < 9; i++) {
            Set s;
            s.tag = i;
            CHECK(s.a.reserve(4 + (size_t)i, nothing()) == hipSuccess && s.h.reserve(2, nothing()) == hipSuccess && s.ev.ensure() == hipSuccess);
            if (i & 1) CHECK(s.b.reserve(3, nothing()) == hipSuccess);
            v.push_back(std::move(s));
            CHECK(s.a.get() == nullptr && s.a.capacity() == 0 && s.h.get() == nullptr && s.ev.get() == nullptr); // NOLINT: the moved-from state is the contract
        }
        CHECK(g_live == 9 * 3 + 4);
        g_log.clear();
        const uint32_t* a5 = v[5].a.get();
        v.erase(v.begin() + 3); // (the recycling of the least recently used set)
        CHECK(g_live == 8 * 3 + 3);
        CHECK(v.size() == 8 && v[2].tag == 2 && v[3].tag == 4 && v[4].tag == 5 && v[4].a.get() == a5 && v[4].a.capacity() == 9);
        for (const Set& s : v) {
            CHECK(s.a.capacity() == 4 + (size_t)s.tag && (s.b.get() != nullptr) == ((s.tag & 1) != 0) && s.ev.get() != nullptr);
            s.a.get()[s.a.capacity() - 1] = 1u; // still the set's own storage
        }
        v.erase(v.begin());
        v.emplace_back();
        CHECK(g_live == 7 * 3 + 3);
    }
    CHECK(g_live == 0);
    g_log.clear();
    {
        // the live and the spare scene arrays of a removal
        DeviceBuf<float> live, spare;
        CHECK(live.reserve(16, nothing()) == hipSuccess && spare.reserve(32, nothing()) == hipSuccess);
        float *pl = live.get(), *ps = spare.get();
        g_log.clear();
        live.swap(spare);
        CHECK(log_is({}) && live.get() == ps && live.capacity() == 32 && spare.get() == pl && spare.capacity() == 16);
        // an outgrown hit buffer that a recorded graph still reads: handed to the retired list, alive until that goes
        std::vector<DeviceBuf<float>> retired;
        retired.push_back(std::move(live));
        CHECK(log_is({}) && live.get() == nullptr && live.capacity() == 0 && retired[0].get() == ps && retired[0].capacity() == 32); // NOLINT
        CHECK(live.reserve(64, after_device()) == hipSuccess && log_is({"hipMalloc 256"})); // (empty: nothing waited for, nothing freed)
        // move assignment releases what the target held
        spare = std::move(live);
        CHECK(log_is({"hipFree"}) && g_last_freed == pl && spare.capacity() == 64 && g_live == 2);
        Event e1, e2;
        CHECK(e1.ensure() == hipSuccess && e1.ensure() == hipSuccess && log_is({"hipEventCreateWithFlags(no timing) 0"}));
        CHECK(e2.ensure(hipEventDefault) == hipSuccess && log_is({"hipEventCreateWithFlags(timing) 0"}));
        hipEvent_t h2 = e2;
        e1 = std::move(e2);
        CHECK(log_is({"hipEventDestroy"}) && e1.get() == h2 && e2.get() == nullptr); // NOLINT
        Stream s1, s2;
        CHECK(s1.get() == nullptr && s1.ensure(hipStreamNonBlocking) == hipSuccess && s1.ensure(hipStreamNonBlocking) == hipSuccess);
        CHECK(log_is({"hipStreamCreateWithFlags(non-blocking) 0"}));
        CHECK(s2.ensure_with_priority(hipStreamNonBlocking, -1) == hipSuccess && log_is({"hipStreamCreateWithPriority 0"}));
        Stream s3(std::move(s1));
        CHECK(s1.get() == nullptr && s3.get() != nullptr && log_is({})); // NOLINT
    }
    CHECK(g_live == 0);
    g_log.clear();
}

void test_adopt()
{
    {
        // the scene store's grow-by-copy: the new array exists while the old one is copied from, then the old one goes -- after the wait
        DeviceBuf<float> arr;
        CHECK(arr.reserve_doubling(10, 1024, nothing()) == hipSuccess);
        arr.get()[9] = 5.0f;
        float* old = arr.get();
        DeviceBuf<float> fresh;
        CHECK(fresh.reserve_doubling(1025, arr.capacity(), nothing()) == hipSuccess && fresh.capacity() == 2048);
        fresh.get()[9] = arr.get()[9];
        float* grown = fresh.get();
        CHECK(g_live == 2);
        g_log.clear();
        arr.adopt(std::move(fresh), after_device());
        CHECK(log_is({"hipDeviceSynchronize", "hipFree"}) && g_last_freed == old);
        CHECK(arr.get() == grown && arr.capacity() == 2048 && arr.get()[9] == 5.0f && fresh.get() == nullptr && fresh.capacity() == 0 && g_live == 1); // NOLINT
        // into an empty buffer: nothing to wait for
        DeviceBuf<float> empty;
        empty.adopt(std::move(arr), after_device());
        CHECK(log_is({}) && empty.get() == grown && arr.get() == nullptr); // NOLINT
    }
    CHECK(g_live == 0);
    g_log.clear();
}

// The counters kernels write (Counter): what the context's seven are made of -- one word, four words, two long words.
template <class T, size_t N>
void counter_case(const char* alloc, const char* zeroed, const char* copied)
{
    hipStream_t s = (hipStream_t)(uintptr_t)0x10;
    {
        Counter<T, N> c;
        T out[N];
        CHECK(c.valid && c.get() == nullptr);
        // no buffer: zeros, and no call
        for (T& w : out) w = 7;
        CHECK(c.read(3, out) == hipSuccess && log_is({}));
        for (const T w : out) CHECK(w == 0);
        // ensure allocates once
        CHECK(c.ensure() == hipSuccess && log_is({alloc}) && c.get() != nullptr && g_live == 1);
        T* first = c.get();
        CHECK(c.ensure() == hipSuccess && c.ensure() == hipSuccess && log_is({}) && c.get() == first);
        // zero: one memset of the whole counter on the stream given
        for (size_t i = 0; i < N; i++) c.get()[i] = (T)(i + 1);
        CHECK(c.zero(s) == hipSuccess && log_is({zeroed}));
        for (size_t i = 0; i < N; i++) CHECK(c.get()[i] == 0);
        // a buffer, valid: set the device, wait for it, copy -- in that order, nothing else
        for (size_t i = 0; i < N; i++) c.get()[i] = (T)(40 + i);
        CHECK(c.read(3, out) == hipSuccess && log_is({"hipSetDevice 3", "hipDeviceSynchronize", copied}));
        for (size_t i = 0; i < N; i++) CHECK(out[i] == (T)(40 + i));
        // not valid: zeros, and no call; valid again: the words are still there
        c.valid = false;
        CHECK(c.read(3, out) == hipSuccess && log_is({}));
        for (const T w : out) CHECK(w == 0);
        c.valid = true;
        CHECK(c.read(0, out) == hipSuccess && log_is({"hipSetDevice 0", "hipDeviceSynchronize", copied}) && out[N - 1] == (T)(40 + N - 1));
        // the copy's error is the read's
        g_copy_result = hipErrorInvalidValue;
        CHECK(c.read(3, out) == hipErrorInvalidValue && log_is({"hipSetDevice 3", "hipDeviceSynchronize", copied}));
        g_copy_result = hipSuccess;
        const Counter<T, N> off(false); // (the context's flagged counters start like this)
        CHECK(!off.valid && off.read(3, out) == hipSuccess && log_is({}));
    }
    CHECK(log_is({"hipFree"}) && g_live == 0);
}

void test_counters()
{
    counter_case<uint32_t, 1>("hipMalloc 4", "hipMemsetAsync(s) 4", "hipMemcpy(to host) 4");
    counter_case<uint32_t, 4>("hipMalloc 16", "hipMemsetAsync(s) 16", "hipMemcpy(to host) 16");
    counter_case<unsigned long long, 2>("hipMalloc 16", "hipMemsetAsync(s) 16", "hipMemcpy(to host) 16");
    // a word inside a larger buffer (the query grid's fallback word): the same three calls
    DeviceBuf<uint32_t> words;
    CHECK(words.reserve(12, nothing()) == hipSuccess);
    words.get()[2] = 9u;
    g_log.clear();
    uint32_t w = 0;
    CHECK(read_words(1, words.get() + 2, 1, &w) == hipSuccess && w == 9u);
    CHECK(log_is({"hipSetDevice 1", "hipDeviceSynchronize", "hipMemcpy(to host) 4"}));
    words.release();
    g_log.clear();
}

} // namespace

int main()
{
    test_reserve();
    test_doubling();
    test_failed_grow();
    test_moves();
    test_adopt();
    test_counters();
    CHECK(g_live == 0);
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("all ownership tests passed\n");
    return 0;
}
