// graph_check.cpp -- csrc/sb_graph_math.h on the host (`make hostcheck`, under AddressSanitizer + UBSan and under
// ThreadSanitizer): the half-edge key of the batch's beam graph.  Stand-alone: nothing here is loaded into Python.
//   1. key -> (particle, beam, side) round-trips over every combination of the corner values of the three fields, no key reaches
//      SBG_NO_KEY or first_key_of(capacity), and the order of two keys as numbers is the order of their (particle, beam, side).
//   2. The bitonic network, pass by pass as the kernel runs it, sorts what std::sort sorts: a star (every half-edge of 4096 beams
//      at particle 0 or at its partner), a lattice, random beams with self-loops, widths 0, 2 and one beam; padded with SBG_NO_KEY.
//   3. lower_bound over the sorted keys gives the prefix sum of the degrees, and [capacity] the number of half-edges.
// Prints "GRAPH_CHECK_OK <keys compared> <scenes sorted>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <tuple>
#include <vector>

#include "sb_graph_math.h"

#define MAXP 1024u
#define MAXB 4096u

static int fail(const char *what, unsigned long a, unsigned long b)
{
    fprintf(stderr, "graph_check: %s (%lu, %lu)\n", what, a, b);
    return 1;
}

struct Beam {
    uint32_t a, b, d;
};

// one scene: keys as the kernel lays them out (two per beam, then the padding), sorted by the network, against std::sort and a
// counted prefix sum
static int check_scene(const std::vector<Beam> &beams)
{
    const uint32_t n_half = 2u * (uint32_t)beams.size(), n = sbg::sort_width(n_half);
    if (n < n_half || (n & (n - 1u)) != 0u || (n_half && n >= 2u * n_half)) return fail("sort_width", n_half, n);
    std::vector<uint32_t> keys(n, SBG_NO_KEY), deg(MAXP + 1u, 0u);
    for (size_t j = 0; j < beams.size(); j++) {
        keys[2 * j] = sbg::key(beams[j].a, beams[j].d, 0u), keys[2 * j + 1] = sbg::key(beams[j].b, beams[j].d, 1u);
        deg[beams[j].a]++, deg[beams[j].b]++;
    }
    std::vector<uint32_t> want(keys);
    std::sort(want.begin(), want.end());
    sbg::bitonic_sort(keys.data(), n);
    if (keys != want) return fail("the network's order differs from std::sort's", n_half, n);
    uint32_t run = 0u;
    for (uint32_t p = 0; p <= MAXP; p++) {
        const uint32_t r = sbg::lower_bound(keys.data(), n, sbg::first_key_of(p));
        if (r != run) return fail("lower_bound is not the prefix sum of the degrees", p, r);
        run += deg[p];
    }
    if (run != n_half) return fail("half-edges", run, n_half);
    return 0;
}

int main()
{
    // ---- 1. the codec over the corners
    const uint32_t ps[] = {0u, 1u, 2u, 63u, 64u, 511u, 512u, MAXP - 2u, MAXP - 1u};
    const uint32_t ds[] = {0u, 1u, 2u, 31u, 32u, 2047u, 2048u, MAXB - 2u, MAXB - 1u};
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> corners;
    for (uint32_t p : ps)
        for (uint32_t d : ds)
            for (uint32_t s = 0; s < 2u; s++) corners.emplace_back(p, d, s);
    unsigned long compared = 0;
    for (const auto &x : corners) {
        const uint32_t k = sbg::key(std::get<0>(x), std::get<1>(x), std::get<2>(x));
        if (sbg::key_particle(k) != std::get<0>(x) || sbg::key_beam(k) != std::get<1>(x) || sbg::key_side(k) != std::get<2>(x))
            return fail("round trip", k, 0);
        if (k >= sbg::first_key_of(MAXP) || sbg::first_key_of(MAXP) >= SBG_NO_KEY || (k >> SBG_KEY_BITS) != 0u) return fail("key range", k, 0);
        if (k < sbg::first_key_of(std::get<0>(x)) || k >= sbg::first_key_of(std::get<0>(x) + 1u)) return fail("first_key_of", k, 0);
        for (const auto &y : corners) {
            const uint32_t l = sbg::key(std::get<0>(y), std::get<1>(y), std::get<2>(y));
            if ((k < l) != (x < y) || (k == l) != (x == y)) return fail("key order is not (particle, beam, side) order", k, l);
            compared++;
        }
    }

    // ---- 2. and 3. scenes, two at a time on two threads: the header keeps no state, which ThreadSanitizer confirms
    std::vector<std::vector<Beam>> scenes;
    scenes.emplace_back(); // no beam
    scenes.push_back({{5u, 3u, 7u}}); // one beam, high endpoint first
    {
        std::vector<Beam> star; // particle 0 joined to every other particle, the rest parallel duplicates, data indices descending
        for (uint32_t j = 0; j < MAXB; j++) star.push_back({0u, 1u + j % (MAXP - 1u), MAXB - 1u - j});
        scenes.push_back(star);
    }
    {
        std::vector<Beam> loops; // every beam from the last particle to itself: the largest degree there is
        for (uint32_t j = 0; j < MAXB; j++) loops.push_back({MAXP - 1u, MAXP - 1u, j});
        scenes.push_back(loops);
    }
    {
        std::vector<Beam> chain; // 65 particles, 64 beams
        for (uint32_t j = 0; j < 64u; j++) chain.push_back({j, j + 1u, j});
        scenes.push_back(chain);
    }
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto rnd = [&seed]() {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(seed >> 33);
    };
    for (uint32_t count : {3u, 299u, 1000u, 2049u, 4095u}) {
        std::vector<uint32_t> idx(MAXB);
        for (uint32_t i = 0; i < MAXB; i++) idx[i] = i;
        for (uint32_t i = MAXB - 1u; i > 0u; i--) std::swap(idx[i], idx[rnd() % (i + 1u)]);
        std::vector<Beam> r;
        for (uint32_t j = 0; j < count; j++) r.push_back({rnd() % MAXP, rnd() % MAXP, idx[j]});
        scenes.push_back(r);
    }
    std::vector<int> bad(scenes.size(), 0);
    auto run = [&](size_t first) {
        for (size_t i = first; i < scenes.size(); i += 2) bad[i] = check_scene(scenes[i]);
    };
    std::thread t0(run, 0), t1(run, 1);
    t0.join();
    t1.join();
    for (size_t i = 0; i < scenes.size(); i++)
        if (bad[i]) return fail("scene", i, scenes[i].size());
    printf("GRAPH_CHECK_OK %lu %zu\n", compared, scenes.size());
    return 0;
}
