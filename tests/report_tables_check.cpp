// The scene tables of the engine's reports (csrc/sb_report_tables.h) on their own.  Reads a scene dumped by
// tests/test_hostcheck_cpu.py, gives it an internal particle order and beam copies of its own (the builder only sees spans), and
// runs the builder with the identity caller-slot map and with a strictly increasing subset that drops every 7th slot.  Checks that
// (1) the tables equal a naive serial build, pinv[pidx[i]] == i and every other entry is "none"; (2) each defect -- a slot >= B, an
// endpoint at a data index with no particle, an endpoint >= np, a copy >= nbeam, a data index >= max_particles -- planted once in
// the first and once in a late range is refused with its kind.  Built with AddressSanitizer + UBSan and with ThreadSanitizer by
// `make hostcheck`.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sb_report_tables.h"
#include "sb_scene_codec.h"

#define CHECK(c)                                                                                \
    do {                                                                                        \
        if (!(c)) {                                                                             \
            fprintf(stderr, "report_tables_check: %s failed (line %d) %s\n", #c, __LINE__, g_what); \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)
static const char *g_what = "";

struct Host {
    uint32_t maxP = 0, nbeam = 0;
    std::vector<uint32_t> pidx, user, copy;
    std::vector<SbHostBeam> beams;
};

static sbq::Defect build(const Host &h, bool subset, std::vector<uint32_t> &pinv, uint32_t *np, std::vector<uint32_t> &tab,
                         unsigned planes = sbq::ENDS | sbq::COPY)
{
    const sbq::Defect d = sbq::invert_particles(h.pidx.data(), h.pidx.size(), h.maxP, pinv, np);
    if (d != sbq::OK) return d;
    return sbq::beam_planes(planes, subset ? h.user.data() : nullptr, subset ? h.user.size() : h.beams.size(), h.beams.data(), h.copy.data(),
                            (uint32_t)h.beams.size(), h.nbeam, pinv, *np, tab);
}

static int refused(const Host &h, bool subset, sbq::Defect want, const char *what)
{
    g_what = what;
    std::vector<uint32_t> pinv, tab;
    uint32_t np = 0;
    const sbq::Defect got = build(h, subset, pinv, &np, tab);
    if (got != want) fprintf(stderr, "%s: got defect %d, want %d\n", what, (int)got, (int)want);
    CHECK(got == want);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    uint32_t head[4]; // layout, max_particles, max_beams, reserved
    std::vector<uint8_t> md(SB_METADATA_BYTES), mp, bd;
    {
        FILE *f = fopen(argv[1], "rb");
        CHECK(f);
        CHECK(fread(head, 4, 4, f) == 4);
        mp.resize(sbc::mapping_bytes(head[0], head[1], head[2]));
        bd.resize((size_t)head[2] * sbc::beam_stride(head[0]));
        CHECK(fread(md.data(), 1, md.size(), f) == md.size());
        CHECK(fread(mp.data(), 1, mp.size(), f) == mp.size());
        CHECK(fseek(f, (long)((size_t)head[1] * SB_PARTICLE_STRIDE), SEEK_CUR) == 0);
        CHECK(fread(bd.data(), 1, bd.size(), f) == bd.size());
        fclose(f);
    }
    const sbc::Header hd(md.data());
    const uint32_t P = hd.P, B = hd.B;
    CHECK(P >= 64 && B >= 64 && head[1] > P);

    // the engine's shadows: internal order = the slots rotated and reversed (any permutation will do), three copies a beam
    Host h;
    h.maxP = head[1];
    h.nbeam = 3u * B + 5u;
    h.beams.resize(B);
    h.copy.resize(B);
    std::vector<uint32_t> data_of_slot, slot_of_data;
    const sbc::SceneError ok = sbc::validate_scene(sbc::Scene{head[0], head[1], head[2], P, B, mp.data(), bd.data()}, data_of_slot, slot_of_data,
                                                   [&](const sbc::BeamSlot &r) {
                                                       SbHostBeam &b = h.beams[r.slot];
                                                       b.a = r.a, b.b = r.b, b.da = r.da, b.db = r.db;
                                                       h.copy[r.slot] = 3u * r.slot + (r.slot & 1u);
                                                   });
    CHECK(ok.kind == sbc::SCENE_OK);
    h.pidx.resize(P);
    for (uint32_t i = 0; i < P; i++) h.pidx[i] = data_of_slot[(P - 1u - i + 17u) % P];
    for (uint32_t s = 0; s < B; s++)
        if (s % 7u != 3u) h.user.push_back(s);

    // ---- (1) against a naive serial build
    uint32_t np_want = 0;
    for (uint32_t i = 0; i < P; i++) np_want = std::max(np_want, h.pidx[i] + 1u);
    for (int subset = 0; subset < 2; subset++) {
        g_what = subset ? "subset" : "identity";
        std::vector<uint32_t> pinv, tab;
        uint32_t np = 0;
        CHECK(build(h, subset != 0, pinv, &np, tab) == sbq::OK);
        CHECK(np == np_want && pinv.size() == np);
        std::vector<uint8_t> named(np, 0);
        for (uint32_t i = 0; i < P; i++) {
            CHECK(pinv[h.pidx[i]] == i);
            named[h.pidx[i]] = 1;
        }
        for (uint32_t d = 0; d < np; d++) CHECK(named[d] || pinv[d] == SBQ_NONE);
        const size_t n = subset ? h.user.size() : B;
        CHECK(tab.size() == 4 * n);
        for (size_t u = 0; u < n; u++) {
            const uint32_t slot = subset ? h.user[u] : (uint32_t)u;
            CHECK(tab[u] == h.beams[slot].da && tab[n + u] == h.beams[slot].db && tab[2 * n + u] == slot && tab[3 * n + u] == h.copy[slot]);
        }
        // the planes asked for apart (bodies reads the first three; body summary adds the fourth later) are the same words
        std::vector<uint32_t> ends, copy;
        CHECK(build(h, subset != 0, pinv, &np, ends, sbq::ENDS) == sbq::OK && build(h, subset != 0, pinv, &np, copy, sbq::COPY) == sbq::OK);
        CHECK(ends.size() == 3 * n && copy.size() == n);
        CHECK(std::equal(ends.begin(), ends.end(), tab.begin()) && std::equal(copy.begin(), copy.end(), tab.begin() + 3 * n));
    }

    // ---- (2) defects, in the first and in a late range of slots / particles
    uint32_t hole = SBQ_NONE; // a data index below np at which no particle lives, if the scene has one
    {
        std::vector<uint32_t> pinv;
        uint32_t np = 0;
        CHECK(sbq::invert_particles(h.pidx.data(), P, h.maxP, pinv, &np) == sbq::OK);
        for (uint32_t d = 0; d < np && hole == SBQ_NONE; d++)
            if (pinv[d] == SBQ_NONE) hole = d;
    }
    int defects = 0;
    for (uint32_t at : {1u, B - 9u}) {
        {
            Host x = h; // a slot >= B (through the caller's map)
            x.user[at < x.user.size() ? at : x.user.size() - 2] = B + 3u;
            if (refused(x, true, sbq::BAD_BEAM_SLOT, "slot >= B")) return 1;
            defects++;
        }
        {
            Host x = h; // an endpoint at a data index with no particle: the scene's own hole, or one made by moving a particle up
            uint32_t d = hole;
            if (d == SBQ_NONE) {
                d = x.beams[at].db;
                for (uint32_t i = 0; i < P; i++)
                    if (x.pidx[i] == d) x.pidx[i] = np_want; // (np grows by one; d is left empty)
                CHECK(np_want < x.maxP);
                for (uint32_t s = 0; s < B; s++) { // keep every other beam whole: only slot `at` may name d
                    if (s == at) continue;
                    if (x.beams[s].da == d) x.beams[s].da = np_want;
                    if (x.beams[s].db == d) x.beams[s].db = np_want;
                }
                if (x.beams[at].da == d) x.beams[at].da = np_want;
            } else x.beams[at].db = d;
            if (refused(x, false, sbq::BAD_ENDPOINT, "endpoint names no particle")) return 1;
            defects++;
        }
        {
            Host x = h; // an endpoint >= np
            x.beams[at].da = np_want;
            if (refused(x, false, sbq::BAD_ENDPOINT, "endpoint >= np")) return 1;
            defects++;
        }
        {
            Host x = h; // a copy >= nbeam
            x.copy[at] = x.nbeam;
            if (refused(x, false, sbq::BAD_COPY, "copy >= nbeam")) return 1;
            defects++;
        }
        {
            Host x = h; // a data index >= max_particles
            x.pidx[at == 1u ? 1u : P - 9u] = x.maxP;
            if (refused(x, false, sbq::BAD_PARTICLE_INDEX, "data index >= max_particles")) return 1;
            defects++;
        }
    }
    printf("REPORT_TABLES_OK %u particles %u beams %d defects\n", P, B, defects);
    return 0;
}
