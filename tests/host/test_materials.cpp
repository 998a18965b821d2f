// test_materials.cpp -- the book of per-object surface attributes and the layout of its device copies (csrc/rtx_materials.hpp), host only:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined tests/host/test_materials.cpp -o test_materials
//   1. random sequences of the book's operations against a naive model of plain vectors: after every operation the values match,
//      each count equals a fresh recount, each generation moved exactly as the operation says, and the flag is as it says;
//   2. refused calls, each leaving the book as it was: a range past the count, n = (size_t)-1, NULL with n > 0, NaN, k < 0 and > 1,
//      ior in (0, 1) and above 4, a slot above the table's count; n = 0 at first == count and -0 as an ior (stored as +0) are taken;
//   3. the refraction book as tests/host/test_refract.cpp stated it before the book existed: accepted calls, stores, counts, the
//      values under rtxplan::plan_removal's renumbering, clear;
//   4. removal against rtxplan::index_after_removal for every subset of a 6-object book, with the slot-above-count query afterwards;
//   5. the layouts: ns = 0 and np = 0, a missing or wrong-sized sorted index, a random permutation, planes beside spheres;
//   6. which generation a recorded graph is stale against.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../raytracing-in-windows-console_amd/csrc/rtx_materials.hpp"

using namespace rtxplan;
using rtxmat::Book;
using rtxmat::Generations;

static int g_failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            if (g_failures < 20) std::printf("FAILED line %d: %s\n", __LINE__, #c); \
            g_failures++;                                           \
        }                                                           \
    } while (0)

// The naive model: plain vectors, the three generations (reflectivity, pattern, refraction) and the flag.
struct Model {
    std::vector<float> k, ior;
    std::vector<uint8_t> slot;
    uint64_t gen[3] = {0, 0, 0};
    bool stale = true;
};

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static bool matches(const Book& b, const Model& m)
{
    if (b.size() != m.k.size() || b.size() != m.slot.size() || b.size() != m.ior.size()) return false;
    uint32_t n_k = 0, n_slot = 0, n_ior = 0;
    for (size_t i = 0; i < b.size(); i++) {
        if (!same_bits(b[i].k, m.k[i]) || b[i].slot != m.slot[i] || !same_bits(b[i].ior, m.ior[i])) return false;
        n_k += m.k[i] > 0.0f ? 1u : 0u;
        n_slot += m.slot[i] != 0 ? 1u : 0u;
        n_ior += m.ior[i] > 0.0f ? 1u : 0u;
    }
    if (b.column(&rtxmat::Surface::k) != m.k || b.column(&rtxmat::Surface::slot) != m.slot || b.column(&rtxmat::Surface::ior) != m.ior) return false;
    const Generations& g = b.generations();
    return b.n_reflective() == n_k && b.n_patterned() == n_slot && b.n_refractive() == n_ior && g.reflectivity == m.gen[0] && g.pattern == m.gen[1] &&
           g.refraction == m.gen[2] && b.stale() == m.stale;
}

static Model model_of(const Book& b)
{
    Model m;
    m.k = b.column(&rtxmat::Surface::k);
    m.slot = b.column(&rtxmat::Surface::slot);
    m.ior = b.column(&rtxmat::Surface::ior);
    m.gen[0] = b.generations().reflectivity;
    m.gen[1] = b.generations().pattern;
    m.gen[2] = b.generations().refraction;
    m.stale = b.stale();
    return m;
}

static size_t lowest_slot_above(const Model& m, size_t count)
{
    for (size_t i = 0; i < m.slot.size(); i++) {
        if (m.slot[i] > count) return i;
    }
    return m.slot.size();
}

// ---------------------------------------------------------------- 1. random sequences

static size_t test_random_sequences()
{
    std::mt19937_64 rng(20240611u);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    size_t ops = 0;
    for (int run = 0; run < 40; run++) {
        Book b;
        Model m;
        size_t table = 0; // the table's count, as the context would hold it
        CHECK(matches(b, m));
        for (int step = 0; step < 150; step++, ops++) {
            const size_t count = m.k.size();
            const unsigned op = (unsigned)(rng() % 16);
            // a range: mostly inside, sometimes past the count
            size_t first = count != 0 ? rng() % (count + 1) : 0, n = rng() % (count - first + 1);
            const bool past = rng() % 8 == 0;
            if (past) n = count - first + 1 + rng() % 3;
            if (op < 4 && count < 40) {
                b.append();
                m.k.push_back(0.0f);
                m.slot.push_back(0);
                m.ior.push_back(0.0f);
                m.stale = true;
            } else if (op == 4 && rng() % 6 == 0) {
                b.clear();
                m.k.clear();
                m.slot.clear();
                m.ior.clear();
                m.gen[0]++, m.gen[1]++, m.gen[2]++;
                m.stale = true;
            } else if (op == 5 || op == 6) {
                std::vector<float> k(n);
                for (float& v : k) v = rng() % 3 == 0 ? 0.0f : (float)(rng() % 1001) / 1000.0f;
                const bool bad = n != 0 && rng() % 8 == 0;
                if (bad) k[rng() % n] = (rng() & 1) ? nan : ((rng() & 1) ? -0.25f : 1.5f);
                const char* f = b.set_reflectivity(first, n, k.data());
                CHECK((f != nullptr) == (past || bad));
                if (!f && n != 0) {
                    for (size_t i = 0; i < n; i++) m.k[first + i] = k[i];
                    m.gen[0]++;
                    m.stale = true;
                }
            } else if (op == 7 || op == 8) {
                std::vector<float> ior(n);
                for (float& v : ior) v = rng() % 3 == 0 ? (rng() & 1 ? 0.0f : -0.0f) : 1.0f + (float)(rng() % 301) * 0.01f;
                const bool bad = n != 0 && rng() % 8 == 0;
                if (bad) ior[rng() % n] = (rng() & 1) ? nan : ((rng() & 1) ? 0.5f : 4.5f);
                const char* f = b.set_refraction(first, n, ior.data());
                CHECK((f != nullptr) == (past || bad));
                if (!f && n != 0) {
                    for (size_t i = 0; i < n; i++) m.ior[first + i] = ior[i] > 0.0f ? ior[i] : 0.0f;
                    m.gen[2]++;
                    m.stale = true;
                }
            } else if (op == 9 || op == 10) {
                const size_t slot = rng() % (table + 2); // (table + 1: above the count)
                const char* f = b.set_slot(first, n, slot, table);
                CHECK((f != nullptr) == (past || slot > table));
                if (!f && n != 0) {
                    for (size_t i = 0; i < n; i++) m.slot[first + i] = (uint8_t)slot;
                    m.gen[1]++;
                    m.stale = true;
                }
            } else if (op == 11) {
                // a new table, as rtx_scene_set_patterns takes it: refused while an object's slot is above its count
                const size_t to = rng() % 5;
                CHECK(b.first_slot_above(to) == lowest_slot_above(m, to));
                if (b.first_slot_above(to) == b.size()) {
                    table = to;
                    b.table_changed();
                    m.gen[1]++;
                    m.stale = true;
                }
            } else if (op == 12) {
                std::vector<uint32_t> gone;
                Model kept;
                for (size_t i = 0; i < count; i++) {
                    if (rng() % 3 == 0) {
                        gone.push_back((uint32_t)i);
                    } else {
                        kept.k.push_back(m.k[i]);
                        kept.slot.push_back(m.slot[i]);
                        kept.ior.push_back(m.ior[i]);
                    }
                }
                b.remove(gone);
                m.k = kept.k;
                m.slot = kept.slot;
                m.ior = kept.ior;
                m.gen[0]++, m.gen[1]++, m.gen[2]++;
                m.stale = true;
            } else if (op == 13) {
                b.order_changed();
                m.stale = true;
            } else if (op >= 14) {
                b.uploaded();
                m.stale = false;
            }
            CHECK(matches(b, m));
        }
    }
    return ops;
}

// ---------------------------------------------------------------- 2. refused calls

static void test_refused_calls()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    Book b;
    for (int i = 0; i < 5; i++) b.append();
    const float k0[2] = {0.25f, 1.0f}, i0[2] = {1.5f, 4.0f};
    CHECK(b.set_reflectivity(1, 2, k0) == nullptr && b.set_refraction(2, 2, i0) == nullptr && b.set_slot(0, 2, 3, 3) == nullptr);
    b.uploaded(); // (a refused call must not set the flag either)
    const Model was = model_of(b);
    CHECK(!was.stale && was.gen[0] == 1 && was.gen[1] == 1 && was.gen[2] == 1 && b.n_reflective() == 2 && b.n_refractive() == 2 && b.n_patterned() == 2);
    const float one[2] = {0.5f, 0.5f}, glass[2] = {1.5f, 1.5f};
    const std::string range = "the range goes past rtx_scene_count";
#define REFUSED(call, text)                            \
    do {                                               \
        const char* f__ = (call);                      \
        CHECK(f__ != nullptr && std::string(f__) == (text)); \
        CHECK(matches(b, was));                        \
    } while (0)
    // a range past the count, and no overflow in first + n
    REFUSED(b.set_reflectivity(4, 2, one), range);
    REFUSED(b.set_reflectivity(6, 0, nullptr), range);
    REFUSED(b.set_reflectivity(0, (size_t)-1, one), range);
    REFUSED(b.set_reflectivity(3, (size_t)-2, one), range);
    REFUSED(b.set_refraction(4, 2, glass), range);
    REFUSED(b.set_refraction(6, 0, nullptr), range);
    REFUSED(b.set_refraction(0, (size_t)-1, glass), range);
    REFUSED(b.set_slot(4, 2, 0, 3), range);
    REFUSED(b.set_slot(6, 0, 0, 3), range);
    REFUSED(b.set_slot(1, (size_t)-1, 0, 3), range);
    REFUSED(b.set_slot(4, 2, 9, 3), range); // (the range is looked at first)
    // NULL with n > 0
    REFUSED(b.set_reflectivity(0, 2, nullptr), "k is NULL");
    REFUSED(b.set_refraction(0, 2, nullptr), "ior is NULL");
    // values: a bad one anywhere refuses the whole call
    for (const float bad : {nan, -nan, inf, -inf, -0.25f, -1.0e-30f, 1.0000001f, 2.0f}) {
        const float first_bad[2] = {bad, 0.5f}, last_bad[2] = {0.5f, bad};
        REFUSED(b.set_reflectivity(0, 2, first_bad), "k must be finite, in [0, 1]");
        REFUSED(b.set_reflectivity(3, 2, last_bad), "k must be finite, in [0, 1]");
    }
    for (const float bad : {nan, inf, -inf, 0.5f, 0.99999994f, 1.0e-30f, 4.0000005f, 100.0f, -1.0f, -1.0e-30f}) {
        const float first_bad[2] = {bad, 1.5f}, last_bad[2] = {1.5f, bad};
        REFUSED(b.set_refraction(0, 2, first_bad), "every value must be 0, or finite and in [1, 4]");
        REFUSED(b.set_refraction(3, 2, last_bad), "every value must be 0, or finite and in [1, 4]");
    }
    REFUSED(b.set_slot(0, 5, 4, 3), "the slot is above the table's count");
    REFUSED(b.set_slot(0, 0, 1, 0), "the slot is above the table's count");
#undef REFUSED
    // good calls at the edges: n = 0 at first == count changes nothing at all; -0 is an ior, stored as +0
    CHECK(b.set_reflectivity(5, 0, nullptr) == nullptr && b.set_refraction(5, 0, nullptr) == nullptr && b.set_slot(5, 0, 3, 3) == nullptr);
    CHECK(b.set_reflectivity(0, 0, one) == nullptr && b.set_refraction(2, 0, glass) == nullptr);
    CHECK(matches(b, was));
    const float edges[2] = {0.0f, 1.0f}, minus_zero[1] = {-0.0f};
    CHECK(b.set_reflectivity(3, 2, edges) == nullptr && b[3].k == 0.0f && b[4].k == 1.0f && b.n_reflective() == 3);
    CHECK(b.set_refraction(2, 1, minus_zero) == nullptr && same_bits(b[2].ior, 0.0f) && b.n_refractive() == 1);
    CHECK(b.stale() && b.generations().reflectivity == 2 && b.generations().refraction == 2 && b.generations().pattern == 1);
    // an empty book
    Book none;
    CHECK(none.set_reflectivity(0, 1, one) != nullptr && none.set_reflectivity(0, 0, nullptr) == nullptr && none.first_slot_above(0) == 0);
    CHECK(matches(none, Model()));
}

// ---------------------------------------------------------------- 3. the refraction book, as test_refract.cpp stated it

// (what rtxrefract::call_fault was: the fault of a call, on a copy)
static const char* refraction_fault(const Book& b, size_t first, size_t n, const float* ior, size_t* bad = nullptr)
{
    Book copy = b;
    const char* f = copy.set_refraction(first, n, ior);
    if (bad) {
        *bad = n;
        if (f && first <= b.size() && n <= b.size() - first) rtxrefract::values_fault(n, ior, bad);
    }
    return f;
}

static std::vector<float> iors_of(const Book& b) { return b.column(&rtxmat::Surface::ior); }

static void test_refraction_book()
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // a call: all or nothing
    Book book;
    for (int i = 0; i < 5; i++) book.append();
    const float two[2] = {1.5f, 0.0f}, with_nan[2] = {1.5f, nan}, low[1] = {0.5f};
    size_t bad = 99;
    CHECK(refraction_fault(book, 0, 2, two, &bad) == nullptr);
    CHECK(refraction_fault(book, 3, 2, two) == nullptr);
    CHECK(refraction_fault(book, 5, 0, nullptr) == nullptr);
    CHECK(refraction_fault(book, 4, 2, two) != nullptr);          // a range past the count
    CHECK(refraction_fault(book, 6, 0, nullptr) != nullptr);
    CHECK(refraction_fault(book, 0, (size_t)-1, two) != nullptr); // (no overflow in first + n)
    CHECK(refraction_fault(book, 0, 2, nullptr) != nullptr);
    CHECK(refraction_fault(book, 0, 2, with_nan, &bad) != nullptr && bad == 1);
    CHECK(refraction_fault(book, 2, 1, low, &bad) != nullptr && bad == 0);
    CHECK(book.set_refraction(0, 2, two) == nullptr);
    CHECK(book.set_refraction(3, 2, two) == nullptr);
    CHECK((iors_of(book) == std::vector<float>{1.5f, 0.0f, 0.0f, 1.5f, 0.0f}) && book.n_refractive() == 2);
    const float back[1] = {0.0f}, minus_zero[1] = {-0.0f};
    CHECK(book.set_refraction(0, 1, back) == nullptr);
    CHECK(book.n_refractive() == 1 && book[0].ior == 0.0f);
    CHECK(refraction_fault(book, 1, 1, minus_zero) == nullptr);
    CHECK(book.set_refraction(1, 1, minus_zero) == nullptr);
    CHECK(book.n_refractive() == 1 && !std::signbit(book[1].ior));
    // removal: the values move with the survivors under the renumbering rule
    std::mt19937_64 rng(5u);
    for (int round = 0; round < 200; round++) {
        const size_t n = 1 + rng() % 40;
        std::vector<uint8_t> kind_of(n);
        std::vector<float> iors(n);
        Book b;
        for (size_t i = 0; i < n; i++) {
            kind_of[i] = rng() % 4 == 0 ? 1 : 2;
            iors[i] = rng() % 3 == 0 ? 1.0f + (float)(rng() % 300) * 0.01f : 0.0f;
            b.append();
        }
        CHECK(b.set_refraction(0, n, iors.data()) == nullptr);
        std::vector<uint32_t> removed;
        for (size_t i = 0; i < n; i++) {
            if (rng() % 3 == 0) removed.push_back((uint32_t)i);
        }
        const RemovalPlan plan = plan_removal(kind_of, removed);
        b.remove(removed);
        const std::vector<float> kept = iors_of(b);
        CHECK(kept == survivors_of(iors, removed));
        CHECK(kept.size() == plan.kind_of.size() && kept.size() == n - removed.size());
        uint32_t want = 0;
        for (size_t i = 0; i < n; i++) {
            const uint32_t j = index_after_removal(removed, (uint32_t)i);
            if (j == kNoIndex) continue;
            CHECK(j < kept.size() && kept[j] == iors[i] && plan.kind_of[j] == kind_of[i]);
            want += iors[i] > 0.0f ? 1u : 0u;
        }
        CHECK(b.n_refractive() == want);
    }
    CHECK((survivors_of(std::vector<float>{0.0f, 1.5f, 0.0f, 4.0f}, std::vector<uint32_t>{0}) == std::vector<float>{1.5f, 0.0f, 4.0f}));
    // clear: no object, no value, nothing refractive; a range past the (empty) count is refused
    book.clear();
    CHECK(book.size() == 0 && book.n_refractive() == 0);
    CHECK(refraction_fault(book, 0, 1, two) != nullptr && refraction_fault(book, 0, 0, nullptr) == nullptr);
}

// ---------------------------------------------------------------- 4. removal, every subset of six

static void test_removal()
{
    const float k[6] = {0.0f, 0.5f, 1.0f, 0.0f, 0.25f, 0.0f}, ior[6] = {1.5f, 0.0f, 0.0f, 4.0f, 1.0f, 0.0f};
    const uint8_t slot[6] = {0, 3, 0, 1, 2, 3};
    for (unsigned subset = 0; subset < 64; subset++) {
        Book b;
        for (int i = 0; i < 6; i++) b.append();
        CHECK(b.set_reflectivity(0, 6, k) == nullptr && b.set_refraction(0, 6, ior) == nullptr);
        for (size_t i = 0; i < 6; i++) CHECK(b.set_slot(i, 1, slot[i], 3) == nullptr);
        b.uploaded();
        const Generations before = b.generations();
        std::vector<uint32_t> removed;
        for (uint32_t i = 0; i < 6; i++) {
            if (subset >> i & 1u) removed.push_back(i);
        }
        b.remove(removed);
        CHECK(b.size() == 6 - removed.size());
        uint32_t n_k = 0, n_slot = 0, n_ior = 0;
        size_t above1 = b.size(), above2 = b.size(); // the lowest survivor with a slot above 1, above 2
        for (uint32_t i = 0; i < 6; i++) {
            const uint32_t j = index_after_removal(removed, i);
            if (j == kNoIndex) continue;
            CHECK(j < b.size() && b[j].k == k[i] && b[j].slot == slot[i] && b[j].ior == ior[i]);
            n_k += k[i] > 0.0f ? 1u : 0u;
            n_slot += slot[i] != 0 ? 1u : 0u;
            n_ior += ior[i] > 0.0f ? 1u : 0u;
            if (slot[i] > 1 && j < above1) above1 = j;
            if (slot[i] > 2 && j < above2) above2 = j;
        }
        CHECK(b.n_reflective() == n_k && b.n_patterned() == n_slot && b.n_refractive() == n_ior);
        CHECK(b.first_slot_above(1) == above1 && b.first_slot_above(2) == above2 && b.first_slot_above(3) == b.size());
        // also a removal of nothing: every generation moves, the flag is set
        const Generations& g = b.generations();
        CHECK(b.stale() && g.reflectivity == before.reflectivity + 1 && g.pattern == before.pattern + 1 && g.refraction == before.refraction + 1);
    }
}

// ---------------------------------------------------------------- 5. the layouts

static void test_layouts()
{
    using rtxmat::layout_of;
    using rtxmat::position_map;
    const std::vector<uint32_t> no_order;
    // no object at all, no sphere, no plane: a single zero where there is nothing
    {
        const auto l = layout_of(std::vector<float>(), {}, {}, 0, 0, no_order);
        CHECK(l.sph == std::vector<float>{0.0f} && l.sph_sorted == l.sph && l.pl == l.sph);
        CHECK(rtxmat::map_stride(0) == 1 && (position_map({}, {}, 0, no_order) == std::vector<uint32_t>{0, 0}));
        const auto planes = layout_of(std::vector<uint8_t>{7, 9}, {1, 1}, {0, 1}, 0, 2, no_order);
        CHECK(planes.sph == std::vector<uint8_t>{0} && planes.sph_sorted == planes.sph && (planes.pl == std::vector<uint8_t>{7, 9}));
        CHECK((position_map({1, 1}, {0, 1}, 0, no_order) == std::vector<uint32_t>{0, 0, 0, 0}));
        const auto spheres = layout_of(std::vector<float>{0.5f, 0.25f}, {2, 2}, {0, 1}, 2, 0, {1, 0});
        CHECK((spheres.sph == std::vector<float>{0.5f, 0.25f}) && (spheres.sph_sorted == std::vector<float>{0.25f, 0.5f}) && spheres.pl == std::vector<float>{0.0f});
    }
    std::mt19937_64 rng(77u);
    for (int round = 0; round < 300; round++) {
        const size_t n = 1 + rng() % 40;
        std::vector<uint8_t> kind_of(n);
        std::vector<uint32_t> local_of(n);
        std::vector<float> value(n);
        uint32_t ns = 0, np = 0;
        for (size_t g = 0; g < n; g++) {
            kind_of[g] = rng() % 4 == 0 ? 1 : 2;
            local_of[g] = kind_of[g] == 2 ? ns++ : np++;
            value[g] = 1.0f + (float)g; // (no zero: a value in the wrong array would show)
        }
        const size_t stride = rtxmat::map_stride(n);
        CHECK(stride == n);
        // without a sorted index, and with one of the wrong size: zeros by sorted position, a map whose halves are equal
        std::vector<uint32_t> wrong(ns + 1 + rng() % 3, 0u);
        if (ns > 1 && (round & 1)) wrong.resize(ns - 1);
        for (const std::vector<uint32_t>* idx : {&no_order, (const std::vector<uint32_t>*)&wrong}) {
            const auto l = layout_of(value, kind_of, local_of, ns, np, *idx);
            const std::vector<uint32_t> map = position_map(kind_of, local_of, ns, *idx);
            CHECK(l.sph.size() == (ns ? ns : 1u) && l.sph_sorted.size() == l.sph.size() && l.pl.size() == (np ? np : 1u) && map.size() == 2 * stride);
            CHECK(l.sph_sorted == std::vector<float>(l.sph.size(), 0.0f));
            for (size_t g = 0; g < n; g++) {
                CHECK((kind_of[g] == 2 ? l.sph : l.pl)[local_of[g]] == value[g]);
                CHECK(map[g] == (kind_of[g] == 2 ? local_of[g] : 0u) && map[stride + g] == map[g]);
            }
        }
        // under a random permutation
        std::vector<uint32_t> idx(ns);
        for (uint32_t p = 0; p < ns; p++) idx[p] = p;
        std::shuffle(idx.begin(), idx.end(), rng);
        const auto l = layout_of(value, kind_of, local_of, ns, np, idx);
        const std::vector<uint32_t> map = position_map(kind_of, local_of, ns, idx);
        for (uint32_t p = 0; p < ns; p++) CHECK(l.sph_sorted[p] == l.sph[idx[p]]);
        if (ns == 0) CHECK(l.sph_sorted == std::vector<float>{0.0f});
        size_t spheres_seen = 0, planes_seen = 0;
        for (size_t g = 0; g < n; g++) {
            if (kind_of[g] == 2) {
                CHECK(map[g] == local_of[g] && map[stride + g] < ns && idx[map[stride + g]] == local_of[g]); // the second half inverts idx
                CHECK(l.sph[local_of[g]] == value[g] && l.sph_sorted[map[stride + g]] == value[g]);
                spheres_seen++;
            } else {
                CHECK(map[g] == 0 && map[stride + g] == 0 && l.pl[local_of[g]] == value[g]);
                planes_seen++;
            }
        }
        // planes never write into sphere arrays, nor spheres into the planes': each array holds its own kind's values and nothing else
        CHECK(spheres_seen == ns && planes_seen == np);
        for (const float v : l.sph) CHECK(ns == 0 ? v == 0.0f : kind_of[(size_t)v - 1] == 2);
        for (const float v : l.pl) CHECK(np == 0 ? v == 0.0f : kind_of[(size_t)v - 1] == 1);
    }
}

// ---------------------------------------------------------------- 6. staleness

static void test_staleness()
{
    Book b;
    b.append();
    const Generations then = b.generations();
    CHECK(rtxmat::stale_fault(then, then) == nullptr && rtxmat::stale_fault(Generations(), Generations()) == nullptr);
    const float k[1] = {0.5f}, ior[1] = {1.5f};
    const auto reason = [&](const Book& now) {
        const char* f = rtxmat::stale_fault(then, now.generations());
        return std::string(f ? f : "");
    };
    const std::string k_text = "the reflectivities changed after this graph was recorded (its launches read the device copies, which the next launch replaces): re-capture";
    const std::string slot_text = "the pattern table or the objects' slots changed after this graph was recorded (its launches read the device copies, which the next launch "
                                  "replaces): re-capture";
    const std::string ior_text = "the indices of refraction changed after this graph was recorded (its launches read the device copies, which the next launch replaces): re-capture";
    Book c = b;
    CHECK(c.set_reflectivity(0, 1, k) == nullptr && reason(c) == k_text);
    c = b;
    CHECK(c.set_slot(0, 1, 0, 0) == nullptr && reason(c) == slot_text);
    c = b;
    c.table_changed();
    CHECK(reason(c) == slot_text);
    c = b;
    CHECK(c.set_refraction(0, 1, ior) == nullptr && reason(c) == ior_text);
    // several: the first in the order reflectivity, pattern, refraction
    CHECK(c.set_slot(0, 1, 0, 0) == nullptr && reason(c) == slot_text);
    CHECK(c.set_reflectivity(0, 1, k) == nullptr && reason(c) == k_text);
    c = b;
    c.remove({});
    CHECK(reason(c) == k_text);
    // what moves no generation
    c = b;
    c.append();
    c.order_changed();
    c.uploaded();
    CHECK(c.set_reflectivity(2, 0, nullptr) == nullptr && reason(c).empty());
}

int main()
{
    const size_t ops = test_random_sequences();
    test_refused_calls();
    test_refraction_book();
    test_removal();
    test_layouts();
    test_staleness();
    if (g_failures != 0) {
        std::printf("%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("all materials tests passed (%zu random operations)\n", ops);
    return 0;
}
