// Unit tests of rtxplan::removal_fault, rtxplan::index_after_removal and rtxplan::plan_removal (csrc/rtx_plan.hpp) -- the host part of
// rtx_scene_remove_objects: the checked, ascending set of removed creation indices, the new kind_of / local_of, the per-kind lists of
// removed local indices the kernel rtx_compact_objects searches, and the rule by which survivors are renumbered -- on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/test_scene_remove.cpp -o t && ./t
// (tests/test_host_scene_remove.py builds and runs it).  No HIP, no GPU.
// The yardstick is a model that erases the objects one by one from a vector of (kind, creation index) and counts.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_plan.hpp"

#include <cstdio>
#include <random>
#include <utility>
#include <vector>

using namespace rtxplan;

static int g_failed = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                 \
        }                                                               \
    } while (0)

// one case: `kinds` by creation index, `picks` the caller's list (a set of valid indices, in any order)
static void check_case(const std::vector<uint8_t>& kinds, const std::vector<unsigned>& picks)
{
    const size_t count = kinds.size();
    std::vector<uint32_t> asc;
    CHECK(removal_fault(count, picks.size(), picks.empty() ? nullptr : picks.data(), asc) == picks.size());
    CHECK(asc.size() == picks.size());
    for (size_t i = 1; i < asc.size(); i++) CHECK(asc[i - 1] < asc[i]);

    // the model: objects as (kind, old creation index), erased one at a time in the caller's order
    std::vector<std::pair<uint8_t, uint32_t>> model;
    std::vector<uint32_t> old_local(count);
    uint32_t seen[3] = {0, 0, 0};
    for (size_t i = 0; i < count; i++) {
        model.push_back({kinds[i], (uint32_t)i});
        old_local[i] = seen[kinds[i]]++;
    }
    std::vector<uint32_t> gone_spheres, gone_planes;
    for (unsigned r : picks) {
        for (size_t j = 0; j < model.size(); j++) {
            if (model[j].second == r) {
                model.erase(model.begin() + (long)j);
                break;
            }
        }
    }
    std::vector<bool> left(count, false);
    for (const auto& m : model) left[m.second] = true;
    for (size_t i = 0; i < count; i++) {
        if (!left[i]) (kinds[i] == 2 ? gone_spheres : gone_planes).push_back(old_local[i]);
    }

    const RemovalPlan plan = plan_removal(kinds, asc);
    CHECK(plan.kind_of.size() == model.size() && plan.local_of.size() == model.size());
    CHECK(plan.removed_spheres == gone_spheres && plan.removed_planes == gone_planes);
    for (size_t i = 1; i < plan.removed_spheres.size(); i++) CHECK(plan.removed_spheres[i - 1] < plan.removed_spheres[i]);
    for (size_t i = 1; i < plan.removed_planes.size(); i++) CHECK(plan.removed_planes[i - 1] < plan.removed_planes[i]);
    uint32_t n_of[3] = {0, 0, 0};
    for (size_t j = 0; j < model.size() && j < plan.kind_of.size(); j++) {
        CHECK(plan.kind_of[j] == model[j].first);
        CHECK(plan.local_of[j] == n_of[model[j].first]);
        n_of[model[j].first]++;
        // the rule: the survivor of old index i is object i - |{r in R : r < i}| now, in creation index and within its kind
        CHECK(index_after_removal(asc, model[j].second) == (uint32_t)j);
        const std::vector<uint32_t>& gone_kind = model[j].first == 2 ? plan.removed_spheres : plan.removed_planes;
        CHECK(index_after_removal(gone_kind, old_local[model[j].second]) == plan.local_of[j]);
    }
    CHECK(plan.ns == n_of[2] && plan.np == n_of[1]);
    CHECK(plan.ns + plan.removed_spheres.size() == seen[2] && plan.np + plan.removed_planes.size() == seen[1]);
    for (unsigned r : picks) CHECK(index_after_removal(asc, r) == kNoIndex);
}

int main()
{
    std::mt19937 rng(20261018u);
    int cases = 0;
    for (int round = 0; round < 1200; round++) {
        const size_t count = round < 40 ? (size_t)round : (size_t)(rng() % 601u);
        const unsigned plane_share = (unsigned)(rng() % 5u); // 0: spheres only ... 4: every kind as likely
        std::vector<uint8_t> kinds(count);
        for (auto& k : kinds) k = (plane_share && rng() % 8u < plane_share * 2u) ? 1 : 2;
        if (round % 97 == 5) std::fill(kinds.begin(), kinds.end(), (uint8_t)1); // planes only
        std::vector<unsigned> all(count);
        for (size_t i = 0; i < count; i++) all[i] = (unsigned)i;
        std::vector<std::vector<unsigned>> sets;
        sets.push_back({});  // nothing
        sets.push_back(all); // everything
        std::vector<unsigned> planes, spheres, random_set, second;
        for (size_t i = 0; i < count; i++) {
            (kinds[i] == 1 ? planes : spheres).push_back((unsigned)i);
            if (rng() % 3u == 0u) random_set.push_back((unsigned)i);
            if (i % 2 == 1) second.push_back((unsigned)i);
        }
        sets.push_back(planes);
        sets.push_back(spheres);
        sets.push_back(random_set);
        sets.push_back(second);
        if (count) {
            sets.push_back({0u});
            sets.push_back({(unsigned)(count - 1)});
            if (count > 1) sets.push_back({(unsigned)(count - 1), 0u});
            sets.push_back({(unsigned)(rng() % count)});
        }
        // one of the sets per round in full, the order shuffled (the caller's list is in any order); the small ones always
        for (size_t s = 0; s < sets.size(); s++) {
            if (sets[s].size() > 2 && s != 1 + (size_t)round % 5u) continue;
            std::shuffle(sets[s].begin(), sets[s].end(), rng);
            check_case(kinds, sets[s]);
            cases++;
        }
    }

    // refused lists: the position of the first entry that is out of range or repeats an earlier one; `ascending` is not to be used then
    {
        std::vector<uint32_t> asc;
        const unsigned past[] = {3u, 10u, 4u};
        CHECK(removal_fault(10, 3, past, asc) == 1);
        const unsigned past_first[] = {0xFFFFFFFFu};
        CHECK(removal_fault(10, 1, past_first, asc) == 0);
        const unsigned last_ok[] = {9u};
        CHECK(removal_fault(10, 1, last_ok, asc) == 1 && asc == std::vector<uint32_t>{9u});
        const unsigned dup[] = {5u, 2u, 7u, 2u, 5u};
        CHECK(removal_fault(10, 5, dup, asc) == 3);
        const unsigned dup_then_past[] = {1u, 1u, 99u};
        CHECK(removal_fault(10, 3, dup_then_past, asc) == 1);
        const unsigned past_then_dup[] = {1u, 99u, 1u};
        CHECK(removal_fault(10, 3, past_then_dup, asc) == 1);
        const unsigned any[] = {0u};
        CHECK(removal_fault(0, 1, any, asc) == 0);        // an empty scene has no index
        CHECK(removal_fault(0, 0, nullptr, asc) == 0 && asc.empty());
        CHECK(removal_fault(7, 0, nullptr, asc) == 0 && asc.empty());
        const unsigned sorted_in[] = {6u, 0u, 3u};
        CHECK(removal_fault(7, 3, sorted_in, asc) == 3 && asc == (std::vector<uint32_t>{0u, 3u, 6u}));
    }
    // the rule by hand: 10 objects, R = {2, 3, 7}
    {
        const std::vector<uint32_t> r = {2u, 3u, 7u};
        const uint32_t want[10] = {0u, 1u, kNoIndex, kNoIndex, 2u, 3u, 4u, kNoIndex, 5u, 6u};
        for (uint32_t i = 0; i < 10; i++) CHECK(index_after_removal(r, i) == want[i]);
        CHECK(index_after_removal({}, 5u) == 5u);
    }
    // by hand: sphere, plane, sphere, sphere, plane; remove objects 1 (the first plane) and 2 (the second sphere)
    {
        const std::vector<uint8_t> kinds = {2, 1, 2, 2, 1};
        const RemovalPlan p = plan_removal(kinds, {1u, 2u});
        CHECK(p.kind_of == (std::vector<uint8_t>{2, 2, 1}));
        CHECK(p.local_of == (std::vector<uint32_t>{0u, 1u, 0u}));
        CHECK(p.removed_spheres == std::vector<uint32_t>{1u} && p.removed_planes == std::vector<uint32_t>{0u});
        CHECK(p.ns == 2 && p.np == 1);
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all scene removal planning tests passed (%d random cases)\n", cases);
    return 0;
}
