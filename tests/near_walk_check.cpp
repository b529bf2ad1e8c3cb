// near_walk_check.cpp -- csrc/sb_near_walk.h on the host: the rings of the engine's proximity queries never leave out
// what the float32 distances of sb_batch_near_math.h would keep or let win.  Built by `make hostcheck` with -ffp-contract=off under
// ASan + UBSan and under TSan.
//   near_walk_check [model [case]]   model: 0 the library's walk; 1 NoLow; 2 StopOnTie; 3 NoSlack (the wrong walks below);
//                                    case: all | low | tie | slack
// On a drawn scene and drawn points, at cells_per_side 1, 2, 3, 64 and the default rule, at max_rings 1, 2 and the default, with and
// without `within`, for every row: the model of sb_nearest.hip -- walls, the walk, the leftover list, or the sweep over everything
// where the walk is not complete -- gives the brute-force key and `within` pair, and its swept verdict is the one an independent
// restatement (the ring of every record from its cell, no cell is enumerated) derives.
// Prints NEAR_WALK_CHECK_OK and its coverage, or the first rows that fail and exits 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../softbody-webgpu_amd/csrc/sb_contact_cells.h" // sb_batch_cell_geometry: the cell side's rule
#include "../softbody-webgpu_amd/csrc/sb_near_walk.h"

// The wrong walks, kept here and out of the library.  NoLow: no extra column and row towards lower x and y.  NoSlack: the bound
// without its 2^-20 bounds term.  Tight: the bound of EXACT arithmetic, L(h) = h cell -- the one bound a float d2 can really tie
// (the library's is padded, so `<` against `<=` cannot be observed on it); TightTie: that bound with `<=` in place of `<`.
struct NoLow : snw::Policy {
    static int64_t low() { return 0; }
};
struct NoSlack : snw::Policy {
    static double slack(double) { return 0.0; }
};
struct Tight : snw::Policy {
    static double slack(double) { return 0.0; }
    static double shrink() { return 1.0; }
};
struct TightTie : Tight {
    static bool below(double d2, double bound2) { return d2 <= bound2; }
};
enum { WALK_RIGHT = 0u, WALK_NO_LOW = 1u, WALK_STOP_ON_TIE = 2u, WALK_NO_SLACK = 3u, WALK_TIGHT = 4u };

template <class Cells, class Best>
static bool walk_as(uint32_t model, const sbn::Probe &p, const srw::Grid &g, uint32_t max_rings, bool within, Cells &&cells, Best &&best, uint32_t *rings)
{
    const uint32_t base = model & 3u;
    if (base == WALK_NO_LOW) return snw::walk<NoLow>(p, g, max_rings, within, cells, best, rings);
    if (base == WALK_NO_SLACK) return snw::walk<NoSlack>(p, g, max_rings, within, cells, best, rings);
    if (base == WALK_STOP_ON_TIE && (model & WALK_TIGHT)) return snw::walk<TightTie>(p, g, max_rings, within, cells, best, rings);
    if (model & WALK_TIGHT) return snw::walk<Tight>(p, g, max_rings, within, cells, best, rings);
    return snw::walk(p, g, max_rings, within, cells, best, rings); // (WALK_STOP_ON_TIE alone: the library's bound, on which it changes nothing)
}

struct Scene {
    float bounds, radius;
    std::vector<srw::Rec> recs;
};
struct Binned {
    srw::Grid g;
    std::vector<std::vector<uint32_t>> bins; // G * G cells and the leftover list
    std::vector<uint32_t> bin_of;            // per record
};
struct Stats {
    uint64_t rows = 0, local = 0, stopped = 0, covered = 0, out_of_rings = 0, outside_gate = 0, leftover_wins = 0, low_beam_wins = 0, slack_beams = 0;
    uint64_t swept = 0, rings = 0, visited = 0, failures = 0;
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
        b.bin_of.push_back(at);
    }
    return b;
}

static uint64_t meet(const sbn::Probe &p, const srw::Rec &c)
{
    const bool beam = (c.index & SRW_KIND_BIT) != 0u;
    if (!(p.mask & (beam ? sbn::MASK_BEAMS : sbn::MASK_PARTICLES))) return SBN_NO_KEY;
    const uint32_t index = c.index & ~SRW_KIND_BIT;
    return beam ? sbn::segment_wide(p, c.ax, c.ay, c.bx, c.by, index) : sbn::particle_wide(p, c.ax, c.ay, index);
}

struct Answer {
    uint64_t key = SBN_NO_KEY;
    uint32_t in_p = 0, in_b = 0;
    void take(const sbn::Probe &p, const srw::Rec &c)
    {
        const uint64_t k = meet(p, c);
        if (k != SBN_NO_KEY) ((c.index & SRW_KIND_BIT) ? in_b : in_p)++;
        key = sbn::nearer(key, k);
    }
    float d2() const { return key == SBN_NO_KEY ? -1.0f : sbn::word_as_float(sbn::key_d2(key)); }
};

static sbn::Probe probe(uint32_t mask, float px, float py, float rmax)
{
    uint32_t w[8] = {mask, sbn::float_as_word(px), sbn::float_as_word(py), sbn::float_as_word(rmax), 0xFFFFFFFFu, 0u, 0u, 0u};
    return sbn::probe_of(w);
}

// the exact distance of a point from a segment, in double
static double segment_distance(const sbn::Probe &p, const srw::Rec &c)
{
    const double ex = (double)c.bx - c.ax, ey = (double)c.by - c.ay, wx = (double)p.px - c.ax, wy = (double)p.py - c.ay;
    const double ee = ex * ex + ey * ey, u = ee > 0.0 ? std::min(1.0, std::max(0.0, (wx * ex + wy * ey) / ee)) : 0.0;
    return hypot(c.ax + u * ex - p.px, c.ay + u * ey - p.py);
}

// The swept verdict restated without enumerating a cell: a record of cell (ix, iy) is seen in ring max(ring(ix - cx), ring(iy - cy)),
// ring(k) = k for k >= 0 and -k - 1 below (the extra column and row); the rings start at the first that holds a cell of the grid.
static bool restated_swept(const Scene &s, const Binned &b, const sbn::Probe &p, uint32_t max_rings, bool within)
{
    if (!snw::local(p, s.bounds)) return true;
    if (!(p.mask & (sbn::MASK_PARTICLES | sbn::MASK_BEAMS)) || b.g.G == 1u) return false;
    const int64_t G = b.g.G, cx = (int64_t)floor((double)p.px / (double)b.g.cell), cy = (int64_t)floor((double)p.py / (double)b.g.cell);
    auto ring = [](int64_t k) { return k >= 0 ? k : -k - 1; };
    auto nearest_ring = [&](int64_t c) { return c >= 0 && c < G ? (int64_t)0 : std::min(ring(0 - c), ring(G - 1 - c)); }; // of the grid's columns (rows)
    const int64_t h0 = std::max(nearest_ring(cx), nearest_ring(cy));
    const int64_t cover = std::max(std::max(ring(0 - cx), ring(G - 1 - cx)), std::max(ring(0 - cy), ring(G - 1 - cy))); // the ring of the farthest cell
    const uint64_t wall = (p.mask & sbn::MASK_WALLS) ? sbn::walls_wide(p, s.bounds) : SBN_NO_KEY;
    for (int64_t h = h0, taken = 1;; h++, taken++) {
        if (h >= cover) return false; // covered
        const double l = ((double)h * b.g.cell - 0x1p-20 * s.bounds) * (1.0 - 0x1p-20), l2 = l > 0.0 ? l * l : -1.0;
        if ((double)p.rmax2 < l2) return false;
        if (!within) {
            uint64_t best = wall;
            for (uint32_t i = 0; i < s.recs.size(); i++) {
                if (b.bin_of[i] == (uint32_t)(G * G)) continue;
                const int64_t ix = b.bin_of[i] % G, iy = b.bin_of[i] / G;
                if (std::max(ring(ix - cx), ring(iy - cy)) <= h) best = sbn::nearer(best, meet(p, s.recs[i]));
            }
            if (best != SBN_NO_KEY && (double)sbn::word_as_float(sbn::key_d2(best)) < l2) return false;
        }
        if (taken >= (int64_t)max_rings) return true;
    }
}

// one row against one binned scene; false: the model's answer is not brute force's
static bool check_row(const Scene &s, const Binned &b, const sbn::Probe &p, uint32_t max_rings, bool within, uint32_t model, Stats &st, const char *what,
                      uint64_t *winner = nullptr)
{
    st.rows++;
    const size_t cells = (size_t)b.g.G * b.g.G;
    const uint64_t wall = (p.mask & sbn::MASK_WALLS) ? sbn::walls_wide(p, s.bounds) : SBN_NO_KEY;
    Answer all;
    for (const srw::Rec &c : s.recs) all.take(p, c);
    all.key = sbn::nearer(all.key, wall);
    Answer got;
    got.key = wall;
    bool swept = true;
    uint32_t rings = 0;
    std::vector<uint8_t> seen(cells, 0);
    int64_t last_low_x = INT64_MIN, last_low_y = INT64_MIN;
    if (snw::local(p, s.bounds)) {
        st.local++;
        swept = !walk_as(
            model, p, b.g, max_rings, within,
            [&](uint32_t first, uint32_t count) {
                for (uint32_t c = first; c < first + count; c++) {
                    if (c >= cells) fprintf(stderr, "%s: cell %u outside the grid\n", what, c), exit(1);
                    if (seen[c]++) fprintf(stderr, "%s: cell %u visited twice\n", what, c), exit(1);
                    st.visited++;
                    for (uint32_t i : b.bins[c]) got.take(p, s.recs[i]);
                }
            },
            [&]() { return got.d2(); }, &rings);
        st.rings += rings;
        if (!swept && b.g.G > 1u && rings) { // what ended it, for the coverage
            const int64_t G = b.g.G, cx = (int64_t)floor((double)p.px / (double)b.g.cell), cy = (int64_t)floor((double)p.py / (double)b.g.cell);
            const int64_t h = snw::first_ring<snw::Policy>(cx, cy, G) + rings - 1;
            last_low_x = cx - h - 1, last_low_y = cy - h - 1;
            if (last_low_x <= 0 && cx + h >= G - 1 && last_low_y <= 0 && cy + h >= G - 1) st.covered++;
            else st.stopped++;
        }
        if (swept) st.out_of_rings++;
    } else {
        st.outside_gate++;
    }
    if (swept) { // the sweep: every record, counted afresh; the walk's keys stay
        st.swept++;
        Answer sweep;
        for (const srw::Rec &c : s.recs) sweep.take(p, c);
        got.key = sbn::nearer(got.key, sweep.key), got.in_p = sweep.in_p, got.in_b = sweep.in_b;
    } else if (p.mask & (sbn::MASK_PARTICLES | sbn::MASK_BEAMS)) {
        Answer left;
        for (uint32_t i : b.bins[cells]) left.take(p, s.recs[i]);
        if (left.key < got.key) st.leftover_wins++;
        got.key = sbn::nearer(got.key, left.key), got.in_p += left.in_p, got.in_b += left.in_b;
    }
    bool ok = true;
    if (got.key != all.key) {
        fprintf(stderr, "LOST %s: G %u max_rings %u the walk's winner %016llx, brute force %016llx\n", what, b.g.G, max_rings, (unsigned long long)got.key,
                (unsigned long long)all.key);
        ok = false;
    }
    if (within && (got.in_p != all.in_p || got.in_b != all.in_b)) {
        fprintf(stderr, "MISCOUNTED %s: G %u max_rings %u within %u %u, brute force %u %u\n", what, b.g.G, max_rings, got.in_p, got.in_b, all.in_p, all.in_b);
        ok = false;
    }
    if (!(model & 7u) && swept != restated_swept(s, b, p, max_rings, within)) {
        fprintf(stderr, "SWEPT %s: G %u max_rings %u the walk says %d\n", what, b.g.G, max_rings, (int)swept);
        ok = false;
    }
    if (winner) *winner = got.key;
    if (!swept && all.key != SBN_NO_KEY && sbn::wide_kind(all.key) == sbn::BEAM) {
        for (uint32_t i = 0; i < s.recs.size(); i++) {
            const srw::Rec &c = s.recs[i];
            if (!(c.index & SRW_KIND_BIT) || (c.index & ~SRW_KIND_BIT) != sbn::wide_index(all.key)) continue;
            if (b.bin_of[i] != cells && ((int64_t)(b.bin_of[i] % b.g.G) == last_low_x || (int64_t)(b.bin_of[i] / b.g.G) == last_low_y)) st.low_beam_wins++;
            const double exact = segment_distance(p, c);
            if ((double)sbn::word_as_float(sbn::key_d2(all.key)) < exact * exact) st.slack_beams++; // the absolute slack at work
        }
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
    // beams without particles at their ends, long enough to reach out of the cell they are recorded in (at 64 cells per side and at
    // the default rule), in every direction
    for (int i = 0; i < 600; i++) {
        const float x = U(rng), y = U(rng), len = 20.0f + 0.01f * U(rng), ang = 6.2831853f * (float)i / 600.0f;
        beam(x, y, std::min(std::max(x + len * cosf(ang), 0.0f), 2048.0f), std::min(std::max(y + len * sinf(ang), 0.0f), 2048.0f));
    }
    // edges of the classification: on x = bounds and y = bounds, on the corners, outside, infinite, NaN
    particle(2048.0f, 700.0f), particle(300.0f, 2048.0f), particle(2048.0f, 2048.0f), particle(0.0f, 0.0f), particle(2048.0f, 0.0f);
    particle(-0.5f, 100.0f), particle(2048.5f, 100.0f), particle(100.0f, -1.0e6f), particle(INFINITY, 5.0f), particle(NAN, NAN), particle(7.0f, -INFINITY);
    // a beam across the whole box, one with an end outside, one with a NaN end, one three cells long
    beam(3.0f, 5.0f, 2040.0f, 2000.0f), beam(100.0f, 100.0f, -5.0f, 100.0f), beam(100.0f, 100.0f, NAN, 100.0f), beam(31.0f, 200.0f, 65.0f, 201.0f);
    return s;
}

static std::vector<sbn::Probe> drawn_rows(const Scene &s, uint32_t seed)
{
    std::mt19937 rng(seed ^ 0x9e3779b9u);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    std::vector<sbn::Probe> rows;
    const float B = s.bounds, masks[5] = {7.0f, 1.0f, 2.0f, 3.0f, 5.0f}, reach[6] = {INFINITY, 0.0f, 2.5f, 40.0f, 100.0f, 700.0f};
    auto mask = [&]() { return (uint32_t)masks[rng() % 5u]; };
    for (int i = 0; i < 500; i++) rows.push_back(probe(mask(), B * (3.0f * U(rng) - 1.0f), B * (3.0f * U(rng) - 1.0f), reach[rng() % 6u])); // anywhere in the gate
    for (int i = 0; i < 500; i++) rows.push_back(probe(mask(), B * U(rng), B * U(rng), reach[rng() % 6u]));                                 // in the box
    for (int i = 0; i < 300; i++) { // on and beside a record
        const srw::Rec &c = s.recs[rng() % s.recs.size()];
        if (!(c.ax == c.ax) || fabsf(c.ax) > 4000.0f || fabsf(c.ay) > 4000.0f) continue;
        rows.push_back(probe(mask(), c.ax + (i % 3 ? 4.0f * (U(rng) - 0.5f) : 0.0f), c.ay + (i % 3 ? 4.0f * (U(rng) - 0.5f) : 0.0f), reach[rng() % 6u]));
    }
    for (int i = 0; i <= 64; i += 2) // on cell borders and corners of 32 (64 cells per side)
        for (float r : {INFINITY, 33.0f, 0.0f}) rows.push_back(probe(7u, 32.0f * i, 32.0f * ((i * 7) % 65), r)), rows.push_back(probe(2u, 32.0f * ((i * 5) % 65), 32.0f * i + 16.0f, r));
    for (float e : {0.0f, 0.25f, -0.25f}) { // on, inside and outside the gate
        rows.push_back(probe(7u, -B + e, 300.0f, INFINITY)), rows.push_back(probe(7u, 300.0f, 2.0f * B - e, 50.0f));
        rows.push_back(probe(3u, 2.0f * B - e, 2.0f * B - e, INFINITY)), rows.push_back(probe(1u, -B + e, -B + e, INFINITY));
    }
    rows.push_back(probe(7u, -3.0f * B, 5.0f * B, INFINITY)), rows.push_back(probe(4u, -3.0f * B, 5.0f, INFINITY)), rows.push_back(probe(4u, 5.0f, 5.0f, 2.0f));
    rows.push_back(probe(1u, 100.0f, -1.0e6f + 3.0f, 10.0f)); // beside the particle far outside: beyond the gate, the sweep finds it
    rows.push_back(probe(1u, -0.25f, 100.5f, 2.0f));          // beside the particle just outside: the leftover list wins
    rows.push_back(probe(2u, 1000.0f, 985.0f, INFINITY));     // beside the beam across the box: the leftover list wins
    return rows;
}

// ---- hand-built scenes
static Scene hand(float bounds, std::initializer_list<srw::Rec> recs) { return Scene{bounds, 10.0f, recs}; }

// bounds 1000, 10 cells of 100.  The point in cell 3; beam 5 from x = 199 to x = 299 crosses cells 1 and 2 and is recorded in cell 1;
// particle 4 at 49 in cell 3.  Without the extra column ring 1 is the cells 2 .. 4: the walk stops on the particle and never sees the
// beam, 2 away.
static bool case_low(uint32_t model, Stats &st)
{
    const Scene s = hand(1000.0f, {srw::Rec{199.0f, 250.0f, 299.0f, 250.0f, 5u | SRW_KIND_BIT, 0u}, srw::Rec{350.0f, 250.0f, 0.0f, 0.0f, 4u, 4u}});
    uint64_t won = SBN_NO_KEY;
    const bool ok = check_row(s, bin(s, 10u), probe(3u, 301.0f, 250.0f, INFINITY), SNW_DEFAULT_RINGS, false, model, st, "low", &won);
    return ok && won == sbn::pack_wide(4.0f, sbn::BEAM, 5u);
}

// bounds 1280, 10 cells of 128.  The point at x = 128 - 2^-17, the last float of cell 0; particle 7 straight above it at 512, in
// ring 4; particle 3 at x = 640, in ring 5, at 512 + 2^-17, which rounds to 512: both d2 are 262144 to the bit, and 3 wins.  At the
// exact bound behind ring 4, (4 * 128)^2, `<` walks on and `<=` stops with 7.
static bool case_tie(uint32_t model, Stats &st)
{
    const float px = nextafterf(128.0f, 0.0f);
    const Scene s = hand(1280.0f, {srw::Rec{px, 576.0f, 0.0f, 0.0f, 7u, 7u}, srw::Rec{640.0f, 64.0f, 0.0f, 0.0f, 3u, 3u}});
    uint64_t won = SBN_NO_KEY;
    const bool ok = check_row(s, bin(s, 10u), probe(1u, px, 64.0f, INFINITY), SNW_DEFAULT_RINGS, false, model | WALK_TIGHT, st, "tie of two particles", &won);
    return ok && won == sbn::pack_wide(262144.0f, sbn::PARTICLE, 3u);
}

// bounds 1000, G cells of fl(1000 / G): coord() rounds x / cell, so the last float below k cell can be recorded in cell k.  Found
// by search over G and k (the first that fits; it is printed): such a particle Y (index 3) in cell k, the point in the last float of cell k - 2, and a particle X (index 7)
// straight above the point with d2(Y) < d2(X) < (cell (1 - 2^-20))^2.  Y is out of ring 1's reach and nearer than one cell: without
// the 2^-20 bounds term the walk stops on X behind ring 1.
static bool case_slack(uint32_t model, Stats &st)
{
    Scene s{1000.0f, 1.0f, {}};
    for (uint32_t G = 60u; G <= 480u; G += 7u) {
        const Binned empty = bin(s, G);
        const float cell = empty.g.cell;
        if (empty.g.G != G) return fprintf(stderr, "slack: the grid is not the one the case was made for\n"), false;
        for (uint32_t k = 4u; k < G; k++) {
            const double kc = (double)k * cell, pc = (double)(k - 1u) * cell;
            float x = (float)kc, px = (float)pc;
            if ((double)x >= kc) x = nextafterf(x, 0.0f);
            if ((double)px >= pc) px = nextafterf(px, 0.0f);
            if (srw::coord(x, cell, G) != k) continue;
            const float vx = x - px, d2y = vx * vx;
            const double l = (double)cell * (1.0 - 0x1p-20), l2 = l * l;
            float t = sqrtf(d2y);
            while (!(t * t > d2y)) t = nextafterf(t, INFINITY);
            if (!((double)d2y < l2 && (double)(t * t) < l2 && t < cell)) continue;
            s.recs = {srw::Rec{x, 0.0f, 0.0f, 0.0f, 3u, 3u}, srw::Rec{px, t, 0.0f, 0.0f, 7u, 7u}};
            uint64_t won = SBN_NO_KEY;
            const bool ok = check_row(s, bin(s, G), probe(1u, px, 0.0f, INFINITY), SNW_DEFAULT_RINGS, false, model, st, "slack", &won);
            if (ok) printf("slack: G %u k %u x %.9g px %.9g\n", G, k, (double)x, (double)px);
            return ok && won == sbn::pack_wide(d2y, sbn::PARTICLE, 3u);
        }
    }
    return fprintf(stderr, "slack: no float below k cell is recorded in cell k\n"), false;
}

int main(int argc, char **argv)
{
    const uint32_t model = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 0) : 0u;
    const std::string which = argc > 2 ? argv[2] : "all";
    Stats st;
    bool ok = true;
    if (which == "all" || which == "low") ok = case_low(model, st) && ok;
    if (which == "all" || which == "tie") ok = case_tie(model, st) && ok;
    if (which == "all" || which == "slack") ok = case_slack(model, st) && ok;
    uint32_t default_G = 0;
    if (which == "all") {
        st = Stats();
        const uint32_t seed = 20311u;
        const Scene s = drawn_scene(seed);
        const std::vector<sbn::Probe> rows = drawn_rows(s, seed);
        for (uint32_t cps : {1u, 2u, 3u, 64u, 0u}) {
            const Binned b = bin(s, cps);
            if (cps == 64u && (b.g.G != 64u || b.bins[64u * 64u].size() < 9u)) fprintf(stderr, "the grid or the leftover list is not what the draw was made for\n"), ok = false;
            if (cps == 0u) default_G = b.g.G;
            for (uint32_t max_rings : {1u, 2u, SNW_DEFAULT_RINGS})
                for (int within = 0; within < 2; within++)
                    for (size_t j = 0; j < rows.size() && st.failures <= 8; j++) {
                        char what[64];
                        snprintf(what, sizeof what, "drawn row %zu within %d", j, within);
                        ok = check_row(s, b, rows[j], max_rings, within != 0, model, st, what) && ok;
                    }
        }
        // the program's own coverage
        if (!(st.stopped >= 1 && st.out_of_rings >= 1 && st.outside_gate >= 1 && st.leftover_wins >= 1 && st.low_beam_wins >= 1 && st.slack_beams >= 1 && st.covered >= 1)) {
            fprintf(stderr, "coverage: stopped %llu out_of_rings %llu outside_gate %llu leftover_wins %llu low_beam_wins %llu slack_beams %llu covered %llu\n",
                    (unsigned long long)st.stopped, (unsigned long long)st.out_of_rings, (unsigned long long)st.outside_gate, (unsigned long long)st.leftover_wins,
                    (unsigned long long)st.low_beam_wins, (unsigned long long)st.slack_beams, (unsigned long long)st.covered);
            ok = false;
        }
    }
    if (!ok) {
        printf("NEAR_WALK_CHECK_FAILED model %u case %s\n", model, which.c_str());
        return 1;
    }
    printf("NEAR_WALK_CHECK_OK model %u case %s default_G %u rows %llu local %llu stopped %llu covered %llu out_of_rings %llu outside_gate %llu leftover_wins %llu "
           "low_beam_wins %llu slack_beams %llu swept %llu cells_per_ring %.2f\n",
           model, which.c_str(), default_G, (unsigned long long)st.rows, (unsigned long long)st.local, (unsigned long long)st.stopped, (unsigned long long)st.covered,
           (unsigned long long)st.out_of_rings, (unsigned long long)st.outside_gate, (unsigned long long)st.leftover_wins, (unsigned long long)st.low_beam_wins,
           (unsigned long long)st.slack_beams, (unsigned long long)st.swept, st.rings ? (double)st.visited / (double)st.rings : 0.0);
    return 0;
}
