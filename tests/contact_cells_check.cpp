// contact_cells_check.cpp -- csrc/sb_contact_cells.h on the host, as the kernels call it (`make hostcheck`, with -ffp-contract=off
// under AddressSanitizer + UBSan and under ThreadSanitizer).  Stand-alone: its own main, seeded scenes, nothing loaded into Python.
//   contact_cells_check
// For every particle of every scene, sb_select_ascending must apply exactly the sorted list of touching partners that a plain loop
// over all particles finds -- over the LDS buckets and over sorted runs, with and without a start `last`, and stopped after m
// partners for every m from 0 to the partner count + 1 (m = 0 is the kernels' own `at >= stop` before they call the driver: it
// applies nothing and runs nothing of the header).  Scenes: G in {1, 2, 3, 7} x P in {1, 2, 5, 64, 300} drawn positions (some
// outside the bounds: the clamp; coincident pairs; one NaN), and rings of exactly 0, 1, 3, 4, 5, 7, 8, 9 and 12 partners around a
// centre in a corner, on an edge and in the middle.  Then the threshold against its expression written out here, the cell rule's
// quoted values, a bucket pushed past its capacity, and the LDS words of the buckets against the indices the helpers touch.
// Prints CONTACT_CELLS_CHECK_OK and its coverage, or the first failures and exits 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <set>
#include <thread>
#include <vector>

#include "sb_contact_cells.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (g_fail++ < 20) {                              \
                fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
                fprintf(stderr, __VA_ARGS__);                 \
                fprintf(stderr, "\n");                        \
            }                                                 \
        }                                                     \
    } while (0)

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// the coordinate map the kernels pair with the cells (sb_grid_coord of sb_physics.h, which needs HIP): monotone, clamped, NaN to 0.
// The header never computes a coordinate; any monotone clamped map over cells at least 2r wide gives the brute-force partners.
static uint32_t coord(float x, float cell, uint32_t n)
{
    const float q = x / cell;
    if (!(q > 0.0f)) return 0u;
    if (q >= (float)n) return n - 1u;
    return (uint32_t)q;
}

struct Scene {
    uint32_t G;
    float cell, radius;
    std::vector<float> x, y;
};
struct Stats {
    uint64_t scenes = 0, particles = 0, walks = 0, partners = 0, clamped = 0, coincident = 0, overflowed_scenes = 0;
    std::set<uint32_t> counts, counts_on_buckets; // partner counts seen; those seen where the buckets were walked
};

// both storage forms of one scene
struct Stored {
    std::vector<uint32_t> cx, cy;
    // sorted runs: the indices by cell, descending inside a cell (the order inside a cell must not matter), end[c]
    std::vector<uint32_t> sorted, end;
    // buckets, as the kernels lay them out: entries, then counts; guard words behind
    std::vector<uint32_t> lds;
    bool overflow = false;
};
#define GUARD 0xA5A5A5A5u
#define GUARD_WORDS 64u

static Stored store(const Scene &s)
{
    Stored st;
    const uint32_t P = (uint32_t)s.x.size(), G = s.G, ncell = G * G;
    st.cx.resize(P), st.cy.resize(P);
    std::vector<std::vector<uint32_t>> bins(ncell);
    for (uint32_t i = 0; i < P; i++) {
        st.cx[i] = coord(s.x[i], s.cell, G), st.cy[i] = coord(s.y[i], s.cell, G);
        bins[st.cy[i] * G + st.cx[i]].push_back(i);
    }
    st.end.resize(ncell);
    for (uint32_t c = 0; c < ncell; c++) {
        for (size_t k = bins[c].size(); k-- > 0;) st.sorted.push_back(bins[c][k]);
        st.end[c] = (uint32_t)st.sorted.size();
    }
    const uint32_t words = sb_bucket_entry_words(G) + sb_bucket_count_words(G);
    st.lds.assign(words + GUARD_WORDS, GUARD);
    uint16_t *ent = (uint16_t *)st.lds.data();
    uint32_t *cnt = st.lds.data() + sb_bucket_entry_words(G);
    for (uint32_t w = 0; w < sb_bucket_count_words(G); w++) cnt[w] = 0u;
    // (pushed from the far end: the entries of a cell are not ascending)
    for (uint32_t i = P; i-- > 0;)
        if (sb_bucket_push(ent, cnt, st.cy[i] * G + st.cx[i], i)) st.overflow = true;
    for (uint32_t c = 0; c < ncell; c++) {
        CHECK(sb_bucket_count(cnt, c) == bins[c].size(), "count of cell %u: %u, %zu pushed", c, sb_bucket_count(cnt, c), bins[c].size());
        if (bins[c].size() > SB_BATCH_CELL_K) CHECK(st.overflow, "cell %u holds %zu and no push said so", c, bins[c].size());
    }
    for (uint32_t w = 0; w < GUARD_WORDS; w++) CHECK(st.lds[words + w] == GUARD, "a push wrote %u words past the buckets", w);
    return st;
}

enum { BUCKETS, RUNS };

// the driver over one storage form: what it applies when apply says stop with the stop_after-th partner.  (A budget of 0 is the
// kernels' `at >= stop`, tested before they call the driver: apply is only asked once it has taken a partner.)
static std::vector<uint32_t> walk(const Scene &s, const Stored &st, int form, uint32_t i, bool from_self, uint32_t stop_after)
{
    const SbTouchTest t = sb_touch_test(s.radius);
    const SbCellWindow win(st.cx[i], st.cy[i], s.G);
    const uint16_t *ent = (const uint16_t *)st.lds.data();
    const uint32_t *cnt = st.lds.data() + sb_bucket_entry_words(s.G);
    std::vector<uint32_t> got;
    if (stop_after == 0u) return got;
    auto offer = [&](SbSelect4 &sel, uint32_t o) {
        if (o == i || !sel.wants(o) || !sb_touch_xy(s.x[i], s.y[i], s.x[o], s.y[o], t.thr, t.two_r)) return;
        sel.insert(o);
    };
    sb_select_ascending(
        from_self, from_self ? i : 0u,
        [&](SbSelect4 &sel) {
            if (form == BUCKETS) {
                sb_bucket_for_window(win, ent, cnt, [&](uint32_t o) { offer(sel, o); });
            } else {
                for (uint32_t yy = win.y0; yy <= win.y1; yy++) {
                    uint32_t from, to;
                    win.run(st.end.data(), yy, &from, &to);
                    for (uint32_t k = from; k < to; k++) offer(sel, st.sorted[k]);
                }
            }
        },
        [&](uint32_t o) {
            got.push_back(o);
            return got.size() < stop_after;
        });
    return got;
}

static void check_scene(const Scene &s, Stats &stats)
{
    const Stored st = store(s);
    const uint32_t P = (uint32_t)s.x.size();
    const SbTouchTest t = sb_touch_test(s.radius);
    stats.scenes++;
    stats.overflowed_scenes += st.overflow ? 1u : 0u;
    for (uint32_t i = 0; i < P; i++) {
        std::vector<uint32_t> all, above; // the plain loop over all particles, ascending
        for (uint32_t o = 0; o < P; o++) {
            if (o == i || !sb_touch_xy(s.x[i], s.y[i], s.x[o], s.y[o], t.thr, t.two_r)) continue;
            all.push_back(o);
            if (o > i) above.push_back(o);
            if (s.x[o] == s.x[i] && s.y[o] == s.y[i]) stats.coincident++;
        }
        stats.particles++;
        stats.partners += all.size();
        stats.counts.insert((uint32_t)all.size());
        if (!st.overflow) stats.counts_on_buckets.insert((uint32_t)all.size());
        const SbCellWindow win(st.cx[i], st.cy[i], s.G);
        if (win.x1 - win.x0 < 2u || win.y1 - win.y0 < 2u) stats.clamped++;
        for (int form = BUCKETS; form <= RUNS; form++) {
            if (form == BUCKETS && st.overflow) continue; // (a full bucket sends the kernels to their loop over everybody)
            for (int from_self = 0; from_self <= 1; from_self++) {
                const std::vector<uint32_t> &want = from_self ? above : all;
                for (uint32_t m = 0; m <= want.size() + 1u; m++) {
                    const std::vector<uint32_t> got = walk(s, st, form, i, from_self != 0, m);
                    const std::vector<uint32_t> head(want.begin(), want.begin() + std::min<size_t>(m, want.size()));
                    stats.walks++;
                    CHECK(got == head, "G %u P %u particle %u form %d from_self %d stop %u: applied %zu partners, want %zu (of %zu)", s.G, P, i, form,
                          from_self, m, got.size(), head.size(), want.size());
                }
            }
        }
    }
}

// P drawn positions over a G x G grid of cells `cell` wide; some outside [0, G * cell], some coincident, one NaN (P >= 5)
static Scene drawn(uint32_t G, uint32_t P, float radius, uint32_t seed)
{
    Scene s;
    s.G = G, s.radius = radius, s.cell = radius * 2.0f * (1.0f + 1.0f / 64.0f);
    std::mt19937 rng(seed);
    // about two particles to a cell's area, over the grid or, where that is smaller, past it (clamped into the edge cells)
    const float span = s.cell * std::max((float)G, ceilf(sqrtf(0.5f * (float)P)));
    std::uniform_real_distribution<float> u(-0.1f * span, 1.1f * span);
    for (uint32_t i = 0; i < P; i++) {
        s.x.push_back(u(rng)), s.y.push_back(u(rng));
        if (i >= 2u && i % 7u == 3u) s.x[i] = s.x[i - 2u], s.y[i] = s.y[i - 2u]; // coincident
    }
    if (P >= 5u) s.x[P / 2u] = nanf("");
    return s;
}

// a centre with exactly k partners on a ring just inside 2r, the centre in the cell (cx, cy) of a G x G grid; `crowd`: the ring
// shrunk into the centre's cell (a full bucket)
static Scene ring(uint32_t G, uint32_t cx, uint32_t cy, uint32_t k, bool crowd)
{
    Scene s;
    s.G = G, s.radius = 10.0f, s.cell = 20.3125f;
    const float ox = ((float)cx + 0.5f) * s.cell, oy = ((float)cy + 0.5f) * s.cell, rr = crowd ? 0.4f * s.cell : 19.5f;
    // (the centre takes a slot in the middle, so partners lie below and above it)
    for (uint32_t j = 0; j < k + 1u; j++) {
        if (j == k / 2u) {
            s.x.push_back(ox), s.y.push_back(oy);
            continue;
        }
        const uint32_t q = j < k / 2u ? j : j - 1u;
        const float a = 6.2831853f * (float)((q * 5u) % std::max(k, 1u)) / (float)std::max(k, 1u) + 0.1f; // (5 is coprime to every k used)
        s.x.push_back(ox + rr * cosf(a)), s.y.push_back(oy + rr * sinf(a));
    }
    return s;
}

static void check_threshold()
{
    const float radii[] = {10.0f, 0.0f, -1.0f, nanf(""), 1e-30f, 1e30f, INFINITY};
    for (float radius : radii) {
        // the oracle: the expression as the kernels carried it before this header
        const float two_r = radius * 2.0f;
        const float thr0 = two_r * two_r * 1.001f;
        uint32_t inf_bits = 0x7f800000u;
        float inf;
        memcpy(&inf, &inf_bits, 4);
        const float thr = (thr0 >= 0x1p-100f && thr0 <= 0x1p100f) ? thr0 : inf;
        const SbTouchTest t = sb_touch_test(radius);
        CHECK(bits(t.two_r) == bits(two_r) && bits(t.thr) == bits(thr), "radius %g: {%08x, %08x}, want {%08x, %08x}", radius, bits(t.two_r), bits(t.thr),
              bits(two_r), bits(thr));
    }
    // the test itself at its edges: 2r apart is no contact, an ulp closer is, one spot is, NaN is not
    const SbTouchTest t = sb_touch_test(10.0f);
    CHECK(!sb_touch_xy(100.0f, 100.0f, 120.0f, 100.0f, t.thr, t.two_r), "2r apart touches");
    CHECK(sb_touch_xy(100.0f, 100.0f, nextafterf(120.0f, 0.0f), 100.0f, t.thr, t.two_r), "an ulp inside 2r does not touch");
    CHECK(sb_touch_xy(5.0f, 7.0f, 5.0f, 7.0f, t.thr, t.two_r), "one spot does not touch");
    CHECK(!sb_touch_xy(5.0f, 7.0f, nanf(""), 7.0f, t.thr, t.two_r) && !sb_touch_xy(nanf(""), 7.0f, 5.0f, 7.0f, t.thr, t.two_r), "NaN touches");
    const SbTouchTest n = sb_touch_test(nanf("")); // (the shortcut off: every comparison with NaN is false)
    CHECK(!sb_touch_xy(5.0f, 7.0f, 5.5f, 7.0f, n.thr, n.two_r) && sb_touch_xy(5.0f, 7.0f, 5.0f, 7.0f, n.thr, n.two_r), "NaN radius");
}

static void check_cell_rule()
{
    CHECK(sb_batch_cell_cap(128u) == 17u && sb_batch_cell_cap(256u) == 25u && sb_batch_cell_cap(1024u) == 50u, "caps %u %u %u", sb_batch_cell_cap(128u),
          sb_batch_cell_cap(256u), sb_batch_cell_cap(1024u));
    CHECK(sb_batch_cell_cap(1u) == 1u, "cap of 1");
    const float bad[] = {0.0f, -1.0f, nanf(""), INFINITY, 1e-30f, 1e30f};
    for (float w : bad) {
        float cell = -7.0f;
        CHECK(sb_batch_cell_geometry(1000.0f, w, 50u, &cell) == 0u, "radius %g gives cells", w);
        CHECK(sb_batch_cell_geometry(w, 10.0f, 50u, &cell) == 0u, "bounds %g gives cells", w);
    }
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> e(-18.0f, 18.0f);
    for (int k = 0; k < 20000; k++) {
        const float bounds = exp2f(e(rng)), radius = exp2f(e(rng));
        const uint32_t cap = 1u + rng() % 64u;
        float cell = 0.0f;
        const uint32_t g = sb_batch_cell_geometry(bounds, radius, cap, &cell);
        CHECK(g >= 1u && g <= cap, "G %u outside 1 .. %u", g, cap);
        CHECK(cell >= radius * 2.0f * (1.0f + 1.0f / 64.0f), "cell %g narrower than the rule at radius %g", cell, radius);
        // G cells cover the bounds up to the one rounding of cell = fl(bounds / G) >= (bounds / G) (1 - 2^-24): in exact
        // arithmetic cell * G >= bounds (1 - 2^-24), and no closer bound holds (15 cells of fl(1000 / 15) = 66.666664 end at
        // 999.99994).  What lies past the last cell is clamped into it, so the ulp costs nothing.
        CHECK((double)cell * (double)g >= (double)bounds * (1.0 - 0x1p-24), "%u cells of %g do not cover %g", g, cell, bounds);
    }
    float cell = 0.0f;
    CHECK(sb_batch_cell_geometry(1000.0f, 10.0f, 50u, &cell) == 49u && sb_batch_cell_geometry(1000.0f, 10.0f, 17u, &cell) == 17u, "the default scene's cells");
}

// the LDS words of the buckets equal what the helpers touch: every cell pushed past its capacity and read back, over a buffer of
// exactly that many words with guards on both sides.  The cells are pushed in ascending and in descending order, and a cell's
// entries must still be untouched when its turn comes: a push past the capacity writes into neither neighbour.
static void check_bucket_words()
{
    static const uint32_t sides[] = {1u, 2u, 3u, 7u, 50u};
    for (uint32_t pass = 0; pass < 10u; pass++) {
        const uint32_t G = sides[pass / 2u];
        const bool descending = pass % 2u != 0u;
        const uint32_t ew = sb_bucket_entry_words(G), cw = sb_bucket_count_words(G), words = ew + cw, ncell = G * G;
        std::vector<uint32_t> buf(GUARD_WORDS + words + GUARD_WORDS, GUARD);
        uint16_t *ent = (uint16_t *)(buf.data() + GUARD_WORDS);
        uint32_t *cnt = buf.data() + GUARD_WORDS + ew;
        for (uint32_t w = 0; w < cw; w++) cnt[w] = 0u;
        for (uint32_t n = 0; n < ncell; n++) {
            const uint32_t c = descending ? ncell - 1u - n : n;
            for (uint32_t w = 0; w < SB_BATCH_CELL_K / 2u; w++)
                CHECK(buf[GUARD_WORDS + c * SB_BATCH_CELL_K / 2u + w] == GUARD, "G %u: cell %u was written before anything was pushed into it", G, c);
            for (uint32_t k = 0; k < SB_BATCH_CELL_K + 3u; k++) {
                const bool full = sb_bucket_push(ent, cnt, c, 0x8000u + c * 8u + k);
                CHECK(full == (k >= SB_BATCH_CELL_K), "G %u cell %u push %u: full %d", G, c, k, (int)full);
            }
        }
        std::vector<bool> touched(words, false);
        for (uint32_t c = 0; c < ncell; c++) {
            CHECK(sb_bucket_count(cnt, c) == SB_BATCH_CELL_K + 3u, "G %u cell %u count %u", G, c, sb_bucket_count(cnt, c));
            const SbBucketWords e = sb_bucket_load(ent, c);
            for (uint32_t j = 0; j < SB_BATCH_CELL_K; j++) {
                CHECK(sb_bucket_entry(e, j) == ((0x8000u + c * 8u + j) & 0xffffu), "G %u cell %u entry %u: %x", G, c, j, sb_bucket_entry(e, j));
                touched[(c * SB_BATCH_CELL_K + j) / 2u] = true;
            }
            touched[ew + (c >> 1)] = true;
        }
        for (uint32_t w = 0; w < words; w++) CHECK(touched[w] && buf[GUARD_WORDS + w] != GUARD, "G %u: word %u of %u is never used", G, w, words);
        for (uint32_t w = 0; w < GUARD_WORDS; w++)
            CHECK(buf[w] == GUARD && buf[GUARD_WORDS + words + w] == GUARD, "G %u: a word outside the %u was written", G, words);
    }
}

int main()
{
    check_threshold();
    check_cell_rule();
    check_bucket_words();
    // the scenes, dealt to two threads: the header keeps no state, which ThreadSanitizer confirms
    std::vector<Scene> scenes;
    uint32_t seed = 1u;
    for (uint32_t G : {1u, 2u, 3u, 7u})
        for (uint32_t P : {1u, 2u, 5u, 64u, 300u}) scenes.push_back(drawn(G, P, 10.0f, seed++));
    for (uint32_t k : {0u, 1u, 3u, 4u, 5u, 7u, 8u, 9u, 12u}) {
        scenes.push_back(ring(7u, 3u, 3u, k, false)); // the middle: no bucket is full
        scenes.push_back(ring(7u, 0u, 0u, k, false)); // a corner: the clamp folds the ring into fewer cells
        scenes.push_back(ring(7u, 6u, 2u, k, false)); // an edge
        scenes.push_back(ring(3u, 1u, 1u, k, false)); // the window is the whole grid
        scenes.push_back(ring(7u, 3u, 3u, k, true));  // crowded into one cell
    }
    Stats stats[2];
    auto run = [&](int half) {
        for (size_t k = half; k < scenes.size(); k += 2) check_scene(scenes[k], stats[half]);
    };
    std::thread t0(run, 0), t1(run, 1);
    t0.join();
    t1.join();
    Stats all = stats[0];
    all.scenes += stats[1].scenes, all.particles += stats[1].particles, all.walks += stats[1].walks, all.partners += stats[1].partners;
    all.clamped += stats[1].clamped, all.coincident += stats[1].coincident, all.overflowed_scenes += stats[1].overflowed_scenes;
    all.counts.insert(stats[1].counts.begin(), stats[1].counts.end());
    all.counts_on_buckets.insert(stats[1].counts_on_buckets.begin(), stats[1].counts_on_buckets.end());
    // the coverage the list above promises
    for (uint32_t k : {0u, 1u, 3u, 4u, 5u, 7u, 8u, 9u, 12u}) CHECK(all.counts.count(k) && all.counts_on_buckets.count(k), "no particle with exactly %u partners (on the buckets: %d)", k, (int)all.counts_on_buckets.count(k));
    CHECK(all.clamped > 0 && all.coincident > 0 && all.overflowed_scenes > 0 && all.overflowed_scenes < all.scenes, "coverage: clamped %llu coincident %llu overflowed %llu",
          (unsigned long long)all.clamped, (unsigned long long)all.coincident, (unsigned long long)all.overflowed_scenes);
    if (g_fail) {
        fprintf(stderr, "%d failures\n", g_fail);
        return 1;
    }
    printf("CONTACT_CELLS_CHECK_OK %llu scenes %llu particles %llu walks %llu partners, %llu clamped windows, %llu coincident, %llu scenes with a full bucket\n",
           (unsigned long long)all.scenes, (unsigned long long)all.particles, (unsigned long long)all.walks, (unsigned long long)all.partners,
           (unsigned long long)all.clamped, (unsigned long long)all.coincident, (unsigned long long)all.overflowed_scenes);
    return 0;
}
