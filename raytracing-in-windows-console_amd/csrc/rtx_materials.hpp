// rtx_materials.hpp -- the surface attributes every object carries by creation index (reflectivity, pattern slot, index of
// refraction, finish, shadow casting), stated once for the host: the book that holds them with their counts, the one upload flag and the generations
// recorded graphs are checked against, and the layout of their device copies.  The book's operations are the only way the library
// changes any of it.  Host only, no HIP header: g++ compiles it on its own (tests/host/test_materials.cpp).
#pragma once

#include "rtx_finish.hpp"
#include "rtx_plan.hpp"
#include "rtx_refract.hpp"

#include <algorithm>
#include <vector>

namespace rtxmat {

// What a recorded graph is stale against, beside the scene generation: a change alters which launches make a frame and what they read.
struct Generations {
    uint64_t reflectivity = 0, pattern = 0, refraction = 0, finish = 0, cast = 0;
};

// NULL, or why a graph recorded at `then` must not be replayed `now`: the first of the five that moved, in this order.
inline const char* stale_fault(const Generations& then, const Generations& now)
{
    if (then.reflectivity != now.reflectivity) return "the reflectivities changed after this graph was recorded (its launches read the device copies, which the next launch replaces): re-capture";
    if (then.pattern != now.pattern) return "the pattern table or the objects' slots changed after this graph was recorded (its launches read the device copies, which the next launch replaces): re-capture";
    if (then.refraction != now.refraction) return "the indices of refraction changed after this graph was recorded (its launches read the device copies, which the next launch replaces): re-capture";
    if (then.finish != now.finish) return "the finishes changed after this graph was recorded (its launches read the device copies, which the next launch replaces): re-capture";
    if (then.cast != now.cast) return "the shadow-casting flags changed after this graph was recorded (its launches read the device copies, which the next launch replaces): re-capture";
    return nullptr;
}

// THE RANGE CHECK of every setter: objects first .. first+n-1 of `count` (no overflow in first + n).
inline const char* range_fault(size_t count, size_t first, size_t n) { return first > count || n > count - first ? "the range goes past rtx_scene_count" : nullptr; }

struct Surface {
    float k = 0.0f;   // reflectivity: 0 matt
    uint8_t slot = 0; // of the pattern table, from 1: 0 plain
    float ior = 0.0f; // index of refraction: 0 a mirror (if k > 0)
    rtx_finish finish = rtxfinish::default_finish(); // ambient, diffuse and specular weight, shininess: the reference's constants
    uint8_t cast = 1; // does the object occlude light in the shadow tests (rtx_scene_set_shadow_casting)?  1: as every object did
};

// Does a value count (n_reflective, n_patterned, n_refractive, n_finished)?
inline bool counts(float v) { return v > 0.0f; }
inline bool counts(uint8_t v) { return v != 0; }
inline bool counts(const rtx_finish& f) { return !rtxfinish::is_default(f); }
// ... and for n_shadowless: the flags that are not the default
inline bool casts_no_shadow(uint8_t cast) { return cast == 0; }

// The book.  Every set_* returns NULL for a good call, else what is wrong with it, and is all or nothing: a refused call has changed
// nothing.  A change sets the flag (the device copies are stale until uploaded()) and moves the generation of what changed; a good
// call with n = 0 changes nothing, and appending moves no generation, because the scene generation covers it.
class Book {
public:
    size_t size() const { return v_.size(); }
    const Surface& operator[](size_t i) const { return v_[i]; }
    uint32_t n_reflective() const { return n_k_; }   // k > 0: while not 0 (or under RTX_OPT_REFLECT_CHECK 2) a frame takes the mirror path
    uint32_t n_patterned() const { return n_slot_; } // slot != 0: while not 0 a frame that would be direct takes the light / shadow path
    uint32_t n_refractive() const { return n_ior_; } // ior > 0: while not 0 the mirror path's launches get the ior arrays
    uint32_t n_finished() const { return n_fin_; }   // finish not the default's bytes: while not 0 a frame that would be direct takes the light / shadow path
    uint32_t n_shadowless() const { return n_nocast_; } // cast == 0: while not 0 the launches that run a shadow test get the flags
    bool stale() const { return stale_; }            // the device copies do not hold these values, this table or this sorted order yet
    const Generations& generations() const { return gen_; }
    template <class T>
    std::vector<T> column(T Surface::*field) const // one attribute by creation index: layout_of's input
    {
        std::vector<T> c;
        for (const Surface& s : v_) c.push_back(s.*field);
        return c;
    }

    void append() { edit().push_back(Surface()); }
    void clear() { keep(std::vector<Surface>()); }
    void remove(const std::vector<uint32_t>& ascending) { keep(rtxplan::survivors_of(v_, ascending)); } // (creation indices: the survivors keep their order)
    void order_changed() { edit(); } // a new direction sort: the copies by sorted position follow it
    void uploaded() { stale_ = false; }
    void table_changed() // (its packed copy travels with the slots: also for a table of none)
    {
        edit();
        gen_.pattern++;
    }

    const char* set_reflectivity(size_t first, size_t n, const float* k)
    {
        if (const char* f = range_fault(size(), first, n)) return f;
        if (n != 0 && k == nullptr) return "k is NULL";
        for (size_t i = 0; i < n; i++) {
            if (!(k[i] >= 0.0f && k[i] <= 1.0f)) return "k must be finite, in [0, 1]";
        }
        return store(&Surface::k, n_k_, gen_.reflectivity, first, n, [&](size_t i) { return k[i]; });
    }

    const char* set_refraction(size_t first, size_t n, const float* ior)
    {
        if (const char* f = range_fault(size(), first, n)) return f;
        if (const char* f = rtxrefract::values_fault(n, ior)) return f;
        return store(&Surface::ior, n_ior_, gen_.refraction, first, n, [&](size_t i) { return ior[i] > 0.0f ? ior[i] : 0.0f; }); // (-0 is stored as 0)
    }

    // (*bad, if given: the first finish of the call that is refused, or n)
    const char* set_finish(size_t first, size_t n, const rtx_finish* finishes, size_t* bad = nullptr)
    {
        if (bad) *bad = n;
        if (const char* f = range_fault(size(), first, n)) return f;
        if (const char* f = rtxfinish::values_fault(n, finishes, bad)) return f;
        return store(&Surface::finish, n_fin_, gen_.finish, first, n, [&](size_t i) { return rtxfinish::stored(finishes[i]); }); // (-0 is stored as 0)
    }

    // (*bad, if given: the first flag of the call that is refused, or n)
    const char* set_shadow_casting(size_t first, size_t n, const uint8_t* casts, size_t* bad = nullptr)
    {
        if (bad) *bad = n;
        if (const char* f = range_fault(size(), first, n)) return f;
        if (n != 0 && casts == nullptr) return "casts is NULL";
        for (size_t i = 0; i < n; i++) {
            if (casts[i] > 1) {
                if (bad) *bad = i;
                return "cast must be 0 or 1";
            }
        }
        return store(&Surface::cast, n_nocast_, gen_.cast, first, n, [&](size_t i) { return casts[i]; }, casts_no_shadow);
    }

    const char* set_slot(size_t first, size_t n, size_t slot, size_t table_count)
    {
        if (const char* f = range_fault(size(), first, n)) return f;
        if (slot > table_count) return "the slot is above the table's count";
        return store(&Surface::slot, n_slot_, gen_.pattern, first, n, [&](size_t) { return (uint8_t)slot; });
    }

    // The lowest object whose slot is above a new table count, or size(): rtx_scene_set_patterns refuses a table that short.
    size_t first_slot_above(size_t table_count) const { return std::find_if(v_.begin(), v_.end(), [&](const Surface& s) { return s.slot > table_count; }) - v_.begin(); }

private:
    std::vector<Surface>& edit() // every write goes through here
    {
        stale_ = true;
        return v_;
    }

    template <class T, class At, class Counts>
    const char* store(T Surface::*field, uint32_t& count, uint64_t& gen, size_t first, size_t n, At value_at, Counts counted)
    {
        for (size_t i = 0; i < n; i++) {
            T& v = edit()[first + i].*field;
            const T to = value_at(i);
            count = count - (counted(v) ? 1u : 0u) + (counted(to) ? 1u : 0u);
            v = to;
        }
        if (n != 0) gen++;
        return nullptr;
    }

    template <class T, class At>
    const char* store(T Surface::*field, uint32_t& count, uint64_t& gen, size_t first, size_t n, At value_at)
    {
        return store(field, count, gen, first, n, value_at, [](const T& v) { return counts(v); });
    }

    void keep(std::vector<Surface> kept) // (every count afresh, every generation moves)
    {
        edit().swap(kept);
        n_k_ = (uint32_t)std::count_if(v_.begin(), v_.end(), [](const Surface& s) { return s.k > 0.0f; });
        n_slot_ = (uint32_t)std::count_if(v_.begin(), v_.end(), [](const Surface& s) { return s.slot != 0; });
        n_ior_ = (uint32_t)std::count_if(v_.begin(), v_.end(), [](const Surface& s) { return s.ior > 0.0f; });
        n_fin_ = (uint32_t)std::count_if(v_.begin(), v_.end(), [](const Surface& s) { return counts(s.finish); });
        n_nocast_ = (uint32_t)std::count_if(v_.begin(), v_.end(), [](const Surface& s) { return casts_no_shadow(s.cast); });
        gen_.reflectivity++;
        gen_.pattern++;
        gen_.refraction++;
        gen_.finish++;
        gen_.cast++;
    }

    std::vector<Surface> v_;
    uint32_t n_k_ = 0, n_slot_ = 0, n_ior_ = 0, n_fin_ = 0, n_nocast_ = 0;
    bool stale_ = true;
    Generations gen_;
};

// One attribute as the kernels index it: spheres by index, spheres by sorted position (sorted_idx: sorted position -> sphere index,
// rtx_sort_scene's; all zeros unless it has exactly ns entries), planes by index -- never fewer than one entry each.
template <class Array> // (std::vector on the host, DeviceBuf on the device)
struct Orders {
    Array sph, sph_sorted, pl;
    const Array& spheres(bool sorted) const { return sorted ? sph_sorted : sph; }
};

template <class T>
inline Orders<std::vector<T>> layout_of(const std::vector<T>& per_object, const std::vector<uint8_t>& kind_of, const std::vector<uint32_t>& local_of, size_t ns, size_t np,
                                        const std::vector<uint32_t>& sorted_idx)
{
    Orders<std::vector<T>> l{std::vector<T>(ns > 0 ? ns : 1, T()), std::vector<T>(ns > 0 ? ns : 1, T()), std::vector<T>(np > 0 ? np : 1, T())};
    for (size_t g = 0; g < per_object.size(); g++) (kind_of[g] == 2 ? l.sph : l.pl)[local_of[g]] = per_object[g];
    for (size_t p = 0; sorted_idx.size() == ns && p < ns; p++) l.sph_sorted[p] = l.sph[sorted_idx[p]];
    return l;
}

// rtx_grid_reflect's map: creation index -> position of the sphere in the scene arrays (words [0, stride)) and in the
// direction-sorted copy (words [stride, 2 stride): the same without a sorted order); a plane's words are 0.
inline size_t map_stride(size_t objects) { return objects > 0 ? objects : 1; }

inline std::vector<uint32_t> position_map(const std::vector<uint8_t>& kind_of, const std::vector<uint32_t>& local_of, size_t ns, const std::vector<uint32_t>& sorted_idx)
{
    const size_t stride = map_stride(kind_of.size());
    const bool sorted = sorted_idx.size() == ns && ns > 0;
    std::vector<uint32_t> pos(2 * stride, 0u), sorted_pos_of(ns, 0u);
    for (size_t p = 0; sorted && p < ns; p++) sorted_pos_of[sorted_idx[p]] = (uint32_t)p;
    for (size_t g = 0; g < kind_of.size(); g++) {
        if (kind_of[g] != 2) continue;
        pos[g] = local_of[g];
        pos[stride + g] = sorted ? sorted_pos_of[local_of[g]] : local_of[g];
    }
    return pos;
}

} // namespace rtxmat
