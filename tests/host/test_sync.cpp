// The stream-ordering contract of csrc/rtx_sync.hpp without a GPU and without a HIP library.  The HIP entry points the header calls
// are defined here as a happens-before model: every fake stream carries a vector clock, a "kernel" ticks its stream's clock,
// hipEventRecord copies the stream's clock into the event, hipStreamWaitEvent joins the event's clock into the stream,
// hipDeviceSynchronize joins everything into everything.  A destroyed stream cannot be recorded on.  Every call is logged.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_sync.hpp"

#include <cstdio>
#include <memory>
#include <random>
#include <string>

namespace {

using Clock = std::vector<long>; // by stream id

void join(Clock& into, const Clock& from)
{
    if (into.size() < from.size()) into.resize(from.size(), 0);
    for (size_t i = 0; i < from.size(); i++) into[i] = into[i] < from[i] ? from[i] : into[i];
}

struct FakeStream {
    size_t id = 0;
    std::string name;
    Clock clock;
    bool destroyed = false;
};

struct FakeEvent {
    Clock clock;
    std::string on = "?"; // the stream it was recorded on last
    bool passed = false;
};

// a launch: the tick it is on its stream, and everything that is known to have finished before it starts
struct Kernel {
    size_t stream = 0;
    long tick = 0;
    Clock before;
};

bool happens_before(const Kernel& a, const Kernel& b) { return a.stream < b.before.size() && b.before[a.stream] >= a.tick; }

std::vector<std::unique_ptr<FakeStream>> g_streams;
std::vector<std::string> g_log;
long g_live_events = 0, g_created_events = 0;
hipError_t g_last = hipSuccess;
int g_failed = 0;

hipStream_t make_stream(const std::string& name)
{
    g_streams.push_back(std::make_unique<FakeStream>());
    FakeStream& s = *g_streams.back();
    s.id = g_streams.size() - 1;
    s.name = name;
    s.clock.assign(s.id + 1, 0);
    return reinterpret_cast<hipStream_t>(&s);
}

FakeStream& fake(hipStream_t s) { return *reinterpret_cast<FakeStream*>(s); }
FakeEvent& fake(hipEvent_t e) { return *reinterpret_cast<FakeEvent*>(e); }

Kernel kernel(hipStream_t on)
{
    FakeStream& s = fake(on);
    Kernel k;
    k.stream = s.id;
    k.before = s.clock;
    k.tick = ++s.clock[s.id];
    return k;
}

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

void reset_model()
{
    g_streams.clear();
    g_log.clear();
    g_last = hipSuccess;
}

} // namespace

extern "C" {
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned)
{
    *e = reinterpret_cast<hipEvent_t>(new FakeEvent);
    g_live_events++;
    g_created_events++;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    delete &fake(e);
    g_live_events--;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    if (!e || fake(s).destroyed) {
        g_log.push_back("record " + fake(s).name + " failed");
        return g_last = hipErrorContextIsDestroyed;
    }
    fake(e).clock = fake(s).clock;
    fake(e).on = fake(s).name;
    fake(e).passed = false;
    g_log.push_back("record " + fake(s).name);
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned)
{
    if (!e || fake(s).destroyed) {
        g_log.push_back("wait " + fake(s).name + " failed");
        return g_last = hipErrorInvalidHandle;
    }
    join(fake(s).clock, fake(e).clock);
    g_log.push_back("wait " + fake(s).name + " " + fake(e).on);
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t e)
{
    g_log.push_back("query");
    return fake(e).passed ? hipSuccess : (g_last = hipErrorNotReady);
}
hipError_t hipDeviceSynchronize(void)
{
    Clock all;
    for (const auto& s : g_streams) join(all, s->clock);
    for (const auto& s : g_streams) join(s->clock, all);
    g_log.push_back("sync");
    return hipSuccess;
}
hipError_t hipGetLastError(void)
{
    g_log.push_back("clear");
    const hipError_t e = g_last;
    g_last = hipSuccess;
    return e;
}
}

using rtxsync::Shared;

namespace {

// ---- the table

struct Entry {
    hipStream_t stream = nullptr;
    int tag = 0;
};

void test_table()
{
    reset_model();
    hipStream_t s[4] = {make_stream("a"), make_stream("b"), make_stream("c"), make_stream("d")};
    std::vector<Entry> v;
    CHECK(rtxsync::find(v, s[0]) == nullptr);
    for (int i = 0; i < 3; i++) {
        Entry* e = rtxsync::add(v, s[i], 3);
        CHECK(e && e->stream == s[i] && e == &v.back());
        e->tag = i + 1;
    }
    CHECK(rtxsync::add(v, s[3], 3) == nullptr && v.size() == 3); // full: the caller decides
    for (int i = 0; i < 3; i++) CHECK(rtxsync::find(v, s[i]) == &v[(size_t)i] && v[(size_t)i].tag == i + 1);
    CHECK(rtxsync::find(v, s[3]) == nullptr);
    v.erase(v.begin()); // (cell_scratch drops the oldest)
    Entry* e = rtxsync::add(v, s[3], 3);
    CHECK(e && e->stream == s[3] && e->tag == 0 && rtxsync::find(v, s[0]) == nullptr && rtxsync::find(v, s[1])->tag == 2);
    CHECK(log_is({}));
}

// ---- scripted sequences: the exact calls, event creation aside.  "wait t s": stream t waits for an event last recorded on s.

// The coarse-cell list cache (rtx_render.cpp: cell_slot_build, cell_slot_use): two sets, render streams s and t, the side stream.
void test_script_cell_cache()
{
    reset_model();
    hipStream_t s = make_stream("s"), t = make_stream("t"), side = make_stream("side");
    {
        Shared A, B;
        CHECK(!A.written() && !A.ready() && log_is({}));
        // the first build, in line on render stream s
        CHECK(A.begin_write(s) == hipSuccess && log_is({}));
        const Kernel w1 = kernel(s);
        CHECK(A.end_write(s, true) == hipSuccess && log_is({"record s"}) && A.written());
        for (int i = 0; i < 3; i++) CHECK(A.read(s) == hipSuccess);
        CHECK(log_is({})); // in order on the stream that built
        CHECK(A.read(t) == hipSuccess && log_is({"wait t s"}));
        const Kernel r1 = kernel(t);
        CHECK(happens_before(w1, r1));
        CHECK(A.read(t) == hipSuccess && A.read(t) == hipSuccess && log_is({})); // once per build
        // a rebuild on s while s and t are open readers: nothing recorded on or waited for on s's own behalf (the build this was
        // taken from also had s wait for its own previous build, a wait that orders nothing)
        CHECK(A.begin_write(s) == hipSuccess && log_is({"record t", "wait s t"}));
        const Kernel w2 = kernel(s);
        CHECK(happens_before(r1, w2) && happens_before(w1, w2));
        CHECK(A.end_write(s, true) == hipSuccess && log_is({"record s"}));
        // t moves from set A to set B
        CHECK(B.begin_write(s) == hipSuccess && B.end_write(s, true) == hipSuccess && log_is({"record s"}));
        CHECK(A.read(t) == hipSuccess && log_is({"wait t s"}));
        const Kernel r2 = kernel(t);
        CHECK(B.read(t) == hipSuccess);
        A.close(t);
        CHECK(log_is({"wait t s", "record t"}));
        A.close(t); // (closed already)
        A.close(side); // (never a reader)
        CHECK(log_is({}));
        const Kernel r3 = kernel(t); // reads B: of no concern to A
        // A is rebuilt ahead of time on the side stream: after its previous build and t's last read of it, without touching t
        CHECK(A.begin_write(side) == hipSuccess && log_is({"wait side s", "wait side t"}));
        const Kernel w3 = kernel(side);
        CHECK(happens_before(r2, w3) && happens_before(w2, w3) && !happens_before(r3, w3));
        CHECK(A.end_write(side, false) == hipSuccess && log_is({"record side"}));
        CHECK(A.last_write() != nullptr && fake(A.last_write()).on == "side");
        CHECK(A.read(s) == hipSuccess && log_is({"wait s side"}));
        CHECK(happens_before(w3, kernel(s)));
        // the side stream itself is not ordered by the flag: a second build there waits for the first
        CHECK(A.begin_write(side) == hipSuccess && log_is({"wait side side", "record s", "wait side s"}));
        CHECK(A.end_write(side, false) == hipSuccess && log_is({"record side"}));
        // buffer growth has waited for the device: nothing to close at the next build
        CHECK(A.read(t) == hipSuccess && log_is({"wait t side"}));
        A.forget_readers();
        CHECK(A.begin_write(s) == hipSuccess && log_is({"wait s side"}));
        CHECK(A.end_write(s, true) == hipSuccess && log_is({"record s"}));
        CHECK(g_created_events == 4 && g_live_events == 4); // two builds' events, s's and t's as readers of A: reused throughout
    }
    CHECK(g_live_events == 0);
    g_created_events = 0;
}

void test_script_ready()
{
    reset_model();
    hipStream_t s = make_stream("s");
    Shared A;
    CHECK(!A.ready() && log_is({})); // never written: nothing to ask
    CHECK(A.begin_write(s) == hipSuccess && A.end_write(s, true) == hipSuccess && log_is({"record s"}));
    CHECK(!A.ready() && log_is({"query", "clear"}));
    fake(A.last_write()).passed = true;
    CHECK(A.ready() && log_is({"query"}));
    CHECK(A.ready() && A.ready() && log_is({})); // cached once true
    CHECK(A.begin_write(s) == hipSuccess && A.end_write(s, true) == hipSuccess && log_is({"record s"}));
    CHECK(!A.ready() && log_is({"query", "clear"})); // a new write: asked again
    g_created_events = 0;
}

// A caller that keeps creating streams: the 33rd distinct one settles everything and starts the table over.
void test_script_overflow()
{
    reset_model();
    hipStream_t s = make_stream("s");
    Shared A;
    CHECK(A.begin_write(s) == hipSuccess);
    const Kernel w1 = kernel(s);
    CHECK(A.end_write(s, true) == hipSuccess && log_is({"record s"}));
    std::vector<Kernel> reads;
    for (size_t i = 1; i < Shared::kMaxReaders; i++) {
        hipStream_t r = make_stream("r" + std::to_string(i));
        CHECK(A.read(r) == hipSuccess);
        reads.push_back(kernel(r));
        CHECK(g_log.size() == 1 && g_log[0] == "wait r" + std::to_string(i) + " s");
        g_log.clear();
    }
    hipStream_t extra = make_stream("extra");
    CHECK(A.read(extra) == hipSuccess && log_is({"sync", "wait extra s"}));
    reads.push_back(kernel(extra));
    CHECK(A.begin_write(s) == hipSuccess && log_is({"wait s s", "record extra", "wait s extra"})); // (s's entry went with the table)
    const Kernel w2 = kernel(s);
    for (const Kernel& r : reads) CHECK(happens_before(w1, r) && happens_before(r, w2));
    g_created_events = 0;
}

void test_script_destroyed_reader()
{
    reset_model();
    hipStream_t s = make_stream("s"), t = make_stream("t");
    Shared A;
    CHECK(A.begin_write(s) == hipSuccess && A.end_write(s, true) == hipSuccess && A.read(t) == hipSuccess);
    const Kernel r = kernel(t);
    fake(t).destroyed = true;
    g_log.clear();
    CHECK(A.begin_write(s) == hipSuccess && log_is({"record t failed", "clear", "sync"}) && g_last == hipSuccess);
    CHECK(happens_before(r, kernel(s)));
    CHECK(A.end_write(s, true) == hipSuccess && log_is({"record s"}));
    CHECK(A.begin_write(s) == hipSuccess && log_is({})); // t is no reader any more
    g_created_events = 0;
}

// The world grid (rtx_query.cpp): built on the context's stream c; queries and frames on c, t and u.
void test_script_grid()
{
    reset_model();
    hipStream_t c = make_stream("c"), t = make_stream("t"), u = make_stream("u");
    Shared G;
    CHECK(G.begin_write(c) == hipSuccess && log_is({}));
    const Kernel w1 = kernel(c);
    CHECK(G.end_write(c, true) == hipSuccess && log_is({"record c"}));
    CHECK(G.read(c) == hipSuccess && log_is({})); // a query on the context's stream
    const Kernel q0 = kernel(c);
    G.close(c);
    CHECK(log_is({"record c"}));
    std::vector<Kernel> frames;
    for (int frame = 0; frame < 3; frame++) {
        for (hipStream_t r : {t, u}) {
            const std::string n = fake(r).name;
            CHECK(G.read(r) == hipSuccess);
            if (frame == 0) CHECK(g_log.size() == 1 && g_log[0] == "wait " + n + " c"); // once per build, not at every call
            else CHECK(g_log.empty());
            g_log.clear();
            frames.push_back(kernel(r));
            CHECK(happens_before(w1, frames.back()));
            G.close(r);
            CHECK(g_log.size() == 1 && g_log[0] == "record " + n);
            g_log.clear();
        }
    }
    // a rebuild with closed readers c, t and u waits for t and u -- for the last launch of EVERY stream that read, not for the
    // most recent reader alone (a query on t, a query on u, RTX_OPT_QUERY_LOAD, another query)
    CHECK(G.begin_write(c) == hipSuccess && log_is({"wait c t", "wait c u"}));
    const Kernel w2 = kernel(c);
    CHECK(happens_before(q0, w2));
    for (const Kernel& f : frames) CHECK(happens_before(f, w2));
    CHECK(G.end_write(c, true) == hipSuccess && log_is({"record c"}));
    CHECK(G.begin_write(c) == hipSuccess && log_is({}) && G.end_write(c, true) == hipSuccess && log_is({"record c"})); // nobody read in between
    g_created_events = 0;
}

// ---- the property: seeded random sequences of what the two users do

struct Model {
    Shared sync;
    std::vector<Kernel> reads, writes; // every reading and every writing kernel so far
    std::vector<hipStream_t> open;     // streams whose last operation on this one was a read
    bool written = false;
};

void forget(std::vector<hipStream_t>& v, hipStream_t s)
{
    for (size_t i = 0; i < v.size(); i++) {
        if (v[i] == s) v.erase(v.begin() + (long)i--);
    }
}

// false: the sequence broke the contract (said on stdout)
bool run_sequence(unsigned seed, size_t n_shared, int n_ops)
{
    reset_model();
    std::mt19937 rng(seed);
    auto pick = [&](size_t n) { return (size_t)(rng() % n); };
    std::vector<hipStream_t> render;
    for (int i = 0; i < 5; i++) render.push_back(make_stream("r" + std::to_string(i)));
    hipStream_t side = make_stream("side");
    std::vector<Model> m(n_shared);
    int bad = 0;
    auto fail = [&](int op, const char* what) {
        if (bad++ == 0) std::printf("FAILED seed %u (%zu shared), operation %d: %s\n", seed, n_shared, op, what);
    };
    for (int op = 0; op < n_ops; op++) {
        Model& x = m[pick(n_shared)];
        hipStream_t r = render[pick(render.size())];
        size_t what = pick(10);
        if (!x.written) what = 9;
        if (what <= 3 || (what == 4 && n_shared == 2)) {
            // a launch that reads x; with two, now and then as the slot switch (the stream's reads of the other one end here)
            if (x.sync.read(r) != hipSuccess) fail(op, "read failed");
            if (what == 4) {
                Model& other = m[&x == &m[0] ? 1 : 0];
                other.sync.close(r);
                forget(other.open, r);
            }
            const Kernel k = kernel(r);
            for (const Kernel& w : x.writes) {
                if (!happens_before(w, k)) fail(op, "a reading kernel queued after end_write does not come after that write's kernels");
            }
            x.reads.push_back(k);
            forget(x.open, r);
            x.open.push_back(r);
        } else if (what <= 6) {
            x.sync.close(r);
            forget(x.open, r);
        } else if (what == 7 && !x.open.empty()) {
            // the caller destroys a stream that is an open reader, and goes on with a new one
            hipStream_t gone = x.open[pick(x.open.size())];
            fake(gone).destroyed = true;
            forget(render, gone);
            for (Model& y : m) forget(y.open, gone);
            render.push_back(make_stream("r" + std::to_string(g_streams.size())));
        } else {
            // a write: on a render stream or on the side stream, with either flag
            hipStream_t w = pick(3) == 0 ? side : r;
            const bool flag = pick(2) == 0;
            if (x.sync.begin_write(w) != hipSuccess) fail(op, "begin_write failed");
            for (int i = 0; i < 2; i++) {
                const Kernel k = kernel(w);
                for (const Kernel& rd : x.reads) {
                    if (!happens_before(rd, k)) fail(op, "a reading kernel queued before begin_write does not come before that write's kernels");
                }
                for (const Kernel& wr : x.writes) {
                    if (!happens_before(wr, k)) fail(op, "a write's kernels do not come after the write before it");
                }
                x.writes.push_back(k);
            }
            if (x.sync.end_write(w, flag) != hipSuccess) fail(op, "end_write failed");
            x.written = true;
            x.open.clear();
        }
    }
    if (g_last != hipSuccess) fail(n_ops, "an error was left uncleared");
    return bad == 0;
}

void test_property()
{
    long sequences = 0, broken = 0;
    for (size_t n_shared = 1; n_shared <= 2; n_shared++) {
        for (unsigned seed = 1; seed <= 2000; seed++) {
            sequences++;
            if (!run_sequence(seed, n_shared, 40)) broken++;
        }
    }
    std::printf("%ld random sequences of 40 operations, %ld broke the contract\n", sequences, broken);
    CHECK(broken == 0);
    CHECK(g_live_events == 0);
}

} // namespace

int main()
{
    test_table();
    test_script_cell_cache();
    test_script_ready();
    test_script_overflow();
    test_script_destroyed_reader();
    test_script_grid();
    test_property();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("all ordering tests passed\n");
    return 0;
}
