// ray_walk_check.cpp -- csrc/sb_ray_walk.h on the host: the walk of the engine's ray casts never leaves out what the
// float32 tests of sb_batch_ray_math.h would meet.  Built by `make hostcheck` with -ffp-contract=off under ASan + UBSan and under TSan.
//   ray_walk_check [model [case]]   model: 0 the library's walk; 1 NoPad; 2 ExitOnTie (the wrong walks below); case: all | pad | tie
// On drawn scenes and rays, at cells_per_side 1, 2, 3, 64 and the default rule, for every walkable row:
//   (a) every record whose test yields a key lies in a cell the walk visits (run to its end) or on the leftover list;
//   (b) the smallest key over what the walk visits before it stops, and the leftovers, is the smallest key over everything.
// Prints RAY_WALK_CHECK_OK and its coverage, or the first rows that fail and exits 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../softbody-webgpu_amd/csrc/sb_contact_cells.h" // sb_batch_cell_geometry: the cell side's rule
#include "../softbody-webgpu_amd/csrc/sb_ray_walk.h"

// The wrong walks, kept here and out of the library.  NoPad: no margin at all.  Tight: the exit bound of EXACT arithmetic,
// (ahead - r) / |d_major| -- right on integer scenes only, and the one bound at which a tie on t can really stand (the library's own
// bound is padded by 2 R, so `<` against `<=` cannot be observed on it).  TightTie: that bound with `<=` in place of `<`.
struct NoPad : srw::Policy {
    static double along(double, double) { return 0.0; }
    static int64_t columns() { return 0; }
    static double across(double) { return 0.0; }
    static int64_t below() { return 0; }
    static int64_t above() { return 0; }
    static bool stops(double t, double ahead, double, double, double dm, double) { return t < ahead / dm; }
};
struct Tight : srw::Policy {
    static bool stops(double t, double ahead, double, double, double dm, double radius) { return t < (ahead - radius) / dm; }
};
struct TightTie : srw::Policy {
    static bool stops(double t, double ahead, double, double, double dm, double radius) { return t <= (ahead - radius) / dm; }
};
enum { WALK_RIGHT = 0u, WALK_NO_PAD = 1u, WALK_EXIT_ON_TIE = 2u, WALK_TIGHT_EXIT = 4u };

template <class Cells, class Best>
static uint32_t walk_as(uint32_t model, const sbr::Ray &r, const srw::Grid &g, Cells &&cells, Best &&best)
{
    if (model & WALK_NO_PAD) return srw::walk<NoPad>(r, g, cells, best);
    if ((model & WALK_TIGHT_EXIT) && (model & WALK_EXIT_ON_TIE)) return srw::walk<TightTie>(r, g, cells, best);
    if (model & WALK_TIGHT_EXIT) return srw::walk<Tight>(r, g, cells, best);
    return srw::walk(r, g, cells, best); // (WALK_EXIT_ON_TIE alone: the library's bound, on which it changes nothing)
}

struct Scene {
    float bounds, radius;
    std::vector<srw::Rec> recs;
};
struct Binned {
    srw::Grid g;
    std::vector<std::vector<uint32_t>> bins; // G * G cells and the leftover list
};
struct Stats {
    uint64_t rows = 0, walkable = 0, hits = 0, slack_hits = 0, exits = 0, far_tangents = 0, leftover_wins = 0, visited_cells = 0, steps = 0;
    uint64_t beam_beats_later_disc = 0, border_rows = 0, failures = 0;
};

static Binned bin(const Scene &s, uint32_t cells_per_side)
{
    Binned b;
    uint32_t particles = 0;
    for (const srw::Rec &c : s.recs) particles += !(c.index & SRW_KIND_BIT);
    float cell = 1.0f;
    const uint32_t G = srw::ordinary(s.bounds, s.radius) ? sb_batch_cell_geometry(s.bounds, s.radius, cells_per_side ? cells_per_side : srw::default_cap(particles), &cell) : 0u;
    b.g = srw::Grid{G ? G : 1u, G ? cell : s.bounds, s.bounds, s.radius};
    b.bins.resize((size_t)b.g.G * b.g.G + 1u);
    for (uint32_t i = 0; i < s.recs.size(); i++) {
        const srw::Rec &c = s.recs[i];
        const uint32_t at = (c.index & SRW_KIND_BIT) ? srw::beam_bin(c.ax, c.ay, c.bx, c.by, b.g) : srw::particle_bin(c.ax, c.ay, b.g);
        b.bins[at].push_back(i);
    }
    return b;
}

static uint64_t meet(const sbr::Ray &r, const srw::Rec &c, float r2)
{
    const bool beam = (c.index & SRW_KIND_BIT) != 0u;
    if (!(r.mask & (beam ? sbr::MASK_BEAMS : sbr::MASK_PARTICLES))) return SBR_NO_KEY;
    const uint32_t index = c.index & ~SRW_KIND_BIT;
    return beam ? sbr::segment_wide(r, c.ax, c.ay, c.bx, c.by, index) : sbr::disc_wide(r, c.ax, c.ay, r2, index);
}

// the exact distance of a centre from the ray's line, in double
static double line_distance(const sbr::Ray &r, const srw::Rec &c)
{
    const double wx = (double)c.ax - r.ox, wy = (double)c.ay - r.oy, dx = r.dx, dy = r.dy;
    return fabs(wx * dy - wy * dx) / sqrt(dx * dx + dy * dy);
}

static sbr::Ray ray(uint32_t mask, float ox, float oy, float dx, float dy, float tmax)
{
    uint32_t w[8] = {mask, sbr::float_as_word(ox), sbr::float_as_word(oy), sbr::float_as_word(dx), sbr::float_as_word(dy), sbr::float_as_word(tmax), 0xFFFFFFFFu, 0u};
    return sbr::ray_of(w);
}

// one row against one binned scene; false: (a) or (b) fails
static bool check_row(const Scene &s, const Binned &b, const sbr::Ray &r, uint32_t model, Stats &st, const char *what, uint64_t *winner = nullptr)
{
    st.rows++;
    if (!srw::walkable(r, s.bounds)) return true; // (the sweep answers it: every record is tested)
    st.walkable++;
    const float r2 = s.radius * s.radius;
    const size_t cells = (size_t)b.g.G * b.g.G;
    uint64_t all = SBR_NO_KEY;
    for (const srw::Rec &c : s.recs) all = sbr::nearer(all, meet(r, c, r2));
    // (a): the walk to its end
    std::vector<uint8_t> seen(cells, 0);
    st.steps += walk_as(
        model, r, b.g,
        [&](uint32_t first, uint32_t count, uint32_t stride) {
            for (uint32_t k = 0, c = first; k < count; k++, c += stride) {
                if (c >= cells) fprintf(stderr, "%s: cell %u outside the grid\n", what, c), exit(1);
                seen[c] = 1;
            }
        },
        []() { return -1.0f; });
    bool ok = true;
    for (size_t c = 0; c < cells; c++) {
        st.visited_cells += seen[c];
        if (seen[c]) continue;
        for (uint32_t i : b.bins[c])
            if (meet(r, s.recs[i], r2) != SBR_NO_KEY) {
                if (ok) fprintf(stderr, "LOST (a) %s: G %u record %u (index %u) in cell %zu is met but not visited\n", what, b.g.G, i, s.recs[i].index & ~SRW_KIND_BIT, c);
                ok = false;
            }
    }
    // (b): the walk as it stops
    uint64_t got = SBR_NO_KEY;
    const uint32_t steps = walk_as(
        model, r, b.g,
        [&](uint32_t first, uint32_t count, uint32_t stride) {
            for (uint32_t k = 0, c = first; k < count; k++, c += stride)
                for (uint32_t i : b.bins[c]) got = sbr::nearer(got, meet(r, s.recs[i], r2));
        },
        [&]() { return got == SBR_NO_KEY ? -1.0f : sbr::word_as_float((uint32_t)(got >> 32)); });
    uint64_t left = SBR_NO_KEY;
    for (uint32_t i : b.bins[cells]) left = sbr::nearer(left, meet(r, s.recs[i], r2));
    if (left < got) st.leftover_wins++;
    got = sbr::nearer(got, left);
    if (got != all) {
        fprintf(stderr, "LOST (b) %s: G %u the walk's winner %016llx, brute force %016llx\n", what, b.g.G, (unsigned long long)got, (unsigned long long)all);
        ok = false;
    }
    if (winner) *winner = got;
    if (!(r.mask & sbr::MASK_BEAMS) && steps < b.g.G && b.g.G > 3u && all != SBR_NO_KEY) st.exits++; // (stopped before the far end of the grid)
    if (all != SBR_NO_KEY) st.hits++;
    // the slack at work: a disc the float test meets although its centre is farther than r from the line, in double
    if (r.mask & sbr::MASK_PARTICLES)
        for (const srw::Rec &c : s.recs)
            if (!(c.index & SRW_KIND_BIT) && meet(r, c, r2) != SBR_NO_KEY && line_distance(r, c) > (double)s.radius) {
                st.slack_hits++;
                const double w = hypot((double)c.ax - r.ox, (double)c.ay - r.oy);
                if (w > 2.0 * s.bounds) st.far_tangents++;
            }
    if (!ok) st.failures++;
    return ok;
}

// ---- the drawn scene: bounds / r = 2^11
static Scene drawn_scene(uint32_t seed)
{
    std::mt19937 rng(seed);
    Scene s{2048.0f, 1.0f, {}};
    std::uniform_real_distribution<float> U(0.0f, 2048.0f), J(-3.0f, 3.0f);
    uint32_t np = 0, nb = 0;
    auto particle = [&](float x, float y) { s.recs.push_back(srw::Rec{x, y, 0.0f, 0.0f, np, np}); return np++; };
    auto beam = [&](float ax, float ay, float bx, float by) { s.recs.push_back(srw::Rec{ax, ay, bx, by, nb++ | SRW_KIND_BIT, 0u}); };
    for (int i = 0; i < 1500; i++) {
        const float x = U(rng), y = U(rng);
        particle(x, y);
        if (i % 2 == 0) { // a short beam to a neighbour that stays in the box
            const float bx = std::min(std::max(x + J(rng), 0.0f), 2048.0f), by = std::min(std::max(y + J(rng), 0.0f), 2048.0f);
            particle(bx, by);
            beam(x, y, bx, by);
        }
    }
    // edges of the classification: on x = bounds and y = bounds, on the corners, outside, infinite, NaN
    particle(2048.0f, 700.0f), particle(300.0f, 2048.0f), particle(2048.0f, 2048.0f), particle(0.0f, 0.0f), particle(2048.0f, 0.0f);
    particle(-0.5f, 100.0f), particle(2048.5f, 100.0f), particle(100.0f, -1.0e6f), particle(INFINITY, 5.0f), particle(NAN, NAN), particle(7.0f, -INFINITY);
    // beams whose boxes span exactly two and exactly three cells at 64 cells per side (32 wide), a beam across the whole box, one
    // with an end outside, one with a NaN end
    beam(33.0f, 40.0f, 63.0f, 41.0f), beam(31.0f, 100.0f, 33.0f, 100.5f), beam(31.0f, 200.0f, 65.0f, 201.0f), beam(500.0f, 31.0f, 500.5f, 65.0f);
    beam(3.0f, 5.0f, 2040.0f, 2000.0f), beam(100.0f, 100.0f, -5.0f, 100.0f), beam(100.0f, 100.0f, NAN, 100.0f);
    // a lattice row: collinear beams along y = 1024.25, which a ray along that line grazes end to end
    for (int i = 0; i < 60; i++) beam(100.0f + 30.0f * i, 1024.25f, 130.0f + 30.0f * i, 1024.25f);
    return s;
}

static bool drawn_rows(const Scene &s, const std::vector<Binned> &grids, uint32_t seed, uint32_t model, Stats &st)
{
    std::mt19937 rng(seed ^ 0x9e3779b9u);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    std::vector<const srw::Rec *> discs;
    for (const srw::Rec &c : s.recs)
        if (!(c.index & SRW_KIND_BIT) && srw::in_grid(c.ax, c.ay, s.bounds)) discs.push_back(&c);
    std::vector<sbr::Ray> rows;
    const float B = s.bounds, r = s.radius, masks[4] = {7.0f, 1.0f, 2.0f, 5.0f};
    auto mask = [&]() { return (uint32_t)masks[rng() % 4u]; };
    for (int i = 0; i < 400; i++) { // anywhere, any direction, short and endless
        const float ang = 6.2831853f * U(rng), len = i % 3 == 0 ? 1.0f : 1.0e-3f + 100.0f * U(rng);
        rows.push_back(ray(mask(), B * (3.0f * U(rng) - 1.0f), B * (3.0f * U(rng) - 1.0f), len * cosf(ang), len * sinf(ang), i % 4 == 0 ? 50.0f * U(rng) : INFINITY));
    }
    for (int i = 0; i < 1200; i++) { // grazing: tangent to a disc, from origins up to the gate's limit away, just inside and just outside r
        const srw::Rec &c = *discs[rng() % discs.size()];
        const float ox = i % 2 ? B * (3.0f * U(rng) - 1.0f) : (i % 4 ? -B : 2.0f * B), oy = i % 2 ? (i % 4 == 1 ? -B : 2.0f * B) : B * (3.0f * U(rng) - 1.0f);
        const double wx = (double)c.ax - ox, wy = (double)c.ay - oy, w = hypot(wx, wy);
        if (w < 4.0 * r) continue;
        const double off = (double)r * (1.0 + (i % 3 - 1) * 1.0e-4 * U(rng)), side = i % 2 ? 1.0 : -1.0;
        const double tx = c.ax + side * off * (-wy / w), ty = c.ay + side * off * (wx / w); // the tangent point, about
        const float scale = i % 5 == 0 ? 37.5f : 1.0f;
        rows.push_back(ray(i % 7 == 0 ? 7u : 1u, ox, oy, (float)((tx - ox) / w) * scale, (float)((ty - oy) / w) * scale, INFINITY));
    }
    const float cell64 = 32.0f;
    for (int i = 0; i < 64; i += 3) { // along cell borders, through cell corners, both majors and both senses
        rows.push_back(ray(mask(), -5.0f, cell64 * i, 1.0f, 0.0f, INFINITY));
        rows.push_back(ray(mask(), cell64 * i, B + 5.0f, 0.0f, -2.0f, INFINITY));
        rows.push_back(ray(mask(), cell64 * i, cell64 * i, 1.0f, 1.0f, INFINITY));
        rows.push_back(ray(mask(), B - cell64 * i, cell64 * i, -1.0f, 1.0f, 300.0f));
    }
    st.border_rows += 4u * 22u;
    rows.push_back(ray(7u, 500.0f, 500.0f, 0.0f, 0.0f, 5.0f)); // a zero direction: not walkable
    for (float e : {0.0f, 1.0f, -1.0f}) { // origins on, just inside and just outside the gate
        rows.push_back(ray(7u, -B + e * 0.25f, 300.0f, 1.0f, 0.01f, INFINITY));
        rows.push_back(ray(7u, 300.0f, 2.0f * B + e * 0.25f, 0.01f, -1.0f, INFINITY));
    }
    rows.push_back(ray(7u, 0.0f, 0.0f, 0x1p-21f, 0.0f, INFINITY)), rows.push_back(ray(7u, 0.0f, 0.0f, 0x1p-20f, 0.0f, INFINITY)); // a below and on the gate
    rows.push_back(ray(7u, 40.0f, 1024.25f, 1.0f, 0.0f, INFINITY)), rows.push_back(ray(2u, 1990.0f, 1024.25f, -3.0f, 0.0f, 20.0f)); // along the lattice row
    rows.push_back(ray(2u, 50.0f, 1024.25f - 950.0f * 0x1p-12f, 1.0f, 0x1p-12f, 10.0f)); // nearly along it
    bool ok = true;
    for (const Binned &b : grids)
        for (size_t j = 0; j < rows.size(); j++) {
            char what[64];
            snprintf(what, sizeof what, "drawn row %zu", j);
            ok &= check_row(s, b, rows[j], model, st, what);
            if (st.failures > 8) return false;
        }
    return ok;
}

// ---- hand-built scenes on integers (bounds 1000, r = 10, 10 cells per side: cells of 100)
static Scene hand(std::initializer_list<srw::Rec> recs) { return Scene{1000.0f, 10.0f, recs}; }

// a disc one row up from the ray's row, 9 from the line: met; a walk without the pad never looks into its row
static bool case_pad(uint32_t model, Stats &st)
{
    const Scene s = hand({srw::Rec{550.0f, 104.0f, 0.0f, 0.0f, 4u, 4u}});
    uint64_t won = SBR_NO_KEY;
    const bool ok = check_row(s, bin(s, 10u), ray(1u, 0.0f, 95.0f, 1.0f, 0.0f, INFINITY), model, st, "pad", &won);
    return ok && sbr::wide_index(won) == 4u && sbr::wide_kind(won) == sbr::PARTICLE;
}

// discs 7 at (98, 56) and 3 at (100, 50) are both met at t = 90, in columns 0 and 1: 3 wins; at the exact exit bound behind
// column 0, (100 - 10) / 1 = 90, `<` walks on and `<=` stops with 7.  And a beam at x = 90 in column 0 against the disc in column 1,
// both met at t = 90: a row with beams never stops early, so no exit rule can fail this one -- it shows that the whole-line walk
// settles the tie by the kind (the disc wins), whatever the order of the visits.
static bool case_tie(uint32_t model, Stats &st)
{
    const Scene s = hand({srw::Rec{98.0f, 56.0f, 0.0f, 0.0f, 7u, 7u}, srw::Rec{100.0f, 50.0f, 0.0f, 0.0f, 3u, 3u}});
    uint64_t won = SBR_NO_KEY;
    bool ok = check_row(s, bin(s, 10u), ray(1u, 0.0f, 50.0f, 1.0f, 0.0f, INFINITY), model | WALK_TIGHT_EXIT, st, "tie of two discs", &won);
    ok = ok && won == sbr::pack_wide(90.0f, sbr::PARTICLE, 3u);
    const Scene m = hand({srw::Rec{90.0f, 40.0f, 90.0f, 60.0f, 5u | SRW_KIND_BIT, 0u}, srw::Rec{100.0f, 50.0f, 0.0f, 0.0f, 3u, 3u}});
    ok = check_row(m, bin(m, 10u), ray(7u, 0.0f, 50.0f, 1.0f, 0.0f, INFINITY), model, st, "tie of a beam and a disc", &won) && ok;
    if (won == sbr::pack_wide(90.0f, sbr::PARTICLE, 3u)) st.beam_beats_later_disc++;
    else ok = false;
    return ok;
}

int main(int argc, char **argv)
{
    const uint32_t model = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 0) : 0u;
    const std::string which = argc > 2 ? argv[2] : "all";
    Stats st;
    bool ok = true;
    if (which == "all" || which == "pad") ok = case_pad(model, st) && ok;
    if (which == "all" || which == "tie") ok = case_tie(model, st) && ok;
    uint32_t default_G = 0;
    if (which == "all") {
        const uint32_t seed = 20281u;
        const Scene s = drawn_scene(seed);
        std::vector<Binned> grids;
        for (uint32_t cps : {1u, 2u, 3u, 64u, 0u}) grids.push_back(bin(s, cps));
        default_G = grids.back().g.G;
        if (grids[3].g.G != 64u || default_G < 8u) fprintf(stderr, "the grids are not the ones the draw was made for: %u %u\n", grids[3].g.G, default_G), ok = false;
        const Binned &b64 = grids[3];
        if (b64.bins[64u * 64u].size() < 9u) fprintf(stderr, "the leftover list misses the planted records\n"), ok = false;
        ok = drawn_rows(s, grids, seed, model, st) && ok;
        // the program's own coverage
        if (!(st.slack_hits >= 1 && st.far_tangents >= 1 && st.exits >= 50 && st.leftover_wins >= 1 && st.walkable < st.rows && st.hits >= 1000)) {
            fprintf(stderr, "coverage: slack_hits %llu far_tangents %llu exits %llu leftover_wins %llu walkable %llu of %llu hits %llu\n",
                    (unsigned long long)st.slack_hits, (unsigned long long)st.far_tangents, (unsigned long long)st.exits, (unsigned long long)st.leftover_wins,
                    (unsigned long long)st.walkable, (unsigned long long)st.rows, (unsigned long long)st.hits);
            ok = false;
        }
    }
    if (!ok) {
        printf("RAY_WALK_CHECK_FAILED model %u case %s\n", model, which.c_str());
        return 1;
    }
    printf("RAY_WALK_CHECK_OK model %u case %s default_G %u rows %llu walkable %llu hits %llu slack_hits %llu far_tangents %llu exits %llu leftover_wins %llu cells_per_step %.2f\n",
           model, which.c_str(), default_G, (unsigned long long)st.rows, (unsigned long long)st.walkable, (unsigned long long)st.hits,
           (unsigned long long)st.slack_hits, (unsigned long long)st.far_tangents, (unsigned long long)st.exits, (unsigned long long)st.leftover_wins,
           st.steps ? (double)st.visited_cells / (double)st.steps : 0.0);
    return 0;
}
