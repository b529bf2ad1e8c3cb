// The two planes sb_forces_device adds to the scene tables of the engine's reports (csrc/sb_report_tables.h), on their own:
// invert_slots (particle mapping slot -> internal particle) and beam_materials ({spring, damp} per caller beam slot).  Scenes of its
// own making (a seeded generator: argv[1] particles, argv[2] beams; a permutation of the slots, a material per beam, a strictly
// increasing caller-slot map that drops every 5th slot), each against brute force; the empty scene; the defects -- a slot >= P, a slot
// two particles claim, a caller slot >= B in the first and in a late range -- refused with their kind.  Built with AddressSanitizer +
// UBSan and with ThreadSanitizer by `make hostcheck`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sb_report_tables.h"

#define CHECK(c)                                                                                   \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            fprintf(stderr, "forces_tables_check: %s failed (line %d) %s\n", #c, __LINE__, g_what); \
            return 1;                                                                              \
        }                                                                                          \
    } while (0)
static const char *g_what = "";

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_seed >> 33);
}

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

int main(int argc, char **argv)
{
    const uint32_t P = argc > 1 ? (uint32_t)atoi(argv[1]) : 1000u, B = argc > 2 ? (uint32_t)atoi(argv[2]) : 3000u;
    CHECK(P >= 16 && B >= 16);

    // ---- the empty scene: one entry of "none", one pair of zeros; nothing is read
    {
        g_what = "empty";
        std::vector<uint32_t> islot;
        std::vector<float> mat;
        CHECK(sbq::invert_slots(nullptr, 0, islot) == sbq::OK && islot.size() == 1 && islot[0] == SBQ_NONE);
        CHECK(sbq::beam_materials(nullptr, 0, nullptr, 0, mat) == sbq::OK && mat.size() == 2 && mat[0] == 0.0f && mat[1] == 0.0f);
    }

    // ---- a permutation of the slots (Fisher-Yates), against brute force
    std::vector<uint32_t> pslot(P);
    for (uint32_t i = 0; i < P; i++) pslot[i] = i;
    for (uint32_t i = P - 1; i > 0; i--) std::swap(pslot[i], pslot[rnd() % (i + 1)]);
    {
        g_what = "invert_slots";
        std::vector<uint32_t> islot;
        CHECK(sbq::invert_slots(pslot.data(), P, islot) == sbq::OK && islot.size() == P);
        uint32_t moved = 0;
        for (uint32_t s = 0; s < P; s++) {
            uint32_t want = SBQ_NONE;
            for (uint32_t i = 0; i < P && want == SBQ_NONE; i++)
                if (pslot[i] == s) want = i;
            CHECK(islot[s] == want && want != SBQ_NONE);
            moved += want != s;
        }
        CHECK(moved > P / 2); // (no identity)
        std::vector<uint32_t> x = pslot;
        x[3] = P; // a slot outside the scene
        CHECK(sbq::invert_slots(x.data(), P, islot) == sbq::BAD_PARTICLE_SLOT);
        x = pslot;
        x[P - 2] = 0xFFFFFFFFu;
        CHECK(sbq::invert_slots(x.data(), P, islot) == sbq::BAD_PARTICLE_SLOT);
        x = pslot;
        x[P - 1] = x[0]; // a slot two particles claim (and one nobody does)
        CHECK(sbq::invert_slots(x.data(), P, islot) == sbq::BAD_PARTICLE_SLOT);
    }

    // ---- a material per engine slot; the identity and a subset of the caller's slots
    std::vector<SbHostBeam> beams(B);
    for (uint32_t s = 0; s < B; s++) {
        memset(&beams[s], 0, sizeof(SbHostBeam));
        for (int k = 0; k < 9; k++) beams[s].f[k] = (float)(rnd() % 100000u) * 0.01f + (float)k * 1000.0f;
        if (s % 97u == 5u) beams[s].f[3] = -0.0f, beams[s].f[4] = __builtin_nanf("");
    }
    std::vector<uint32_t> user;
    for (uint32_t s = 0; s < B; s++)
        if (s % 5u != 2u) user.push_back(s);
    int defects = 0;
    for (int subset = 0; subset < 2; subset++) {
        g_what = subset ? "materials, subset" : "materials, identity";
        const size_t n = subset ? user.size() : B;
        std::vector<float> mat;
        CHECK(sbq::beam_materials(subset ? user.data() : nullptr, n, beams.data(), B, mat) == sbq::OK && mat.size() == 2 * n);
        for (size_t u = 0; u < n; u++) {
            const uint32_t slot = subset ? user[u] : (uint32_t)u;
            CHECK(same_bits(mat[2 * u], beams[slot].f[3]) && same_bits(mat[2 * u + 1], beams[slot].f[4]));
        }
        if (subset) CHECK(user[7] != 7u); // (no identity)
        for (size_t at : {(size_t)1, user.size() - 3}) { // a caller slot outside the scene, early and late
            std::vector<uint32_t> x = user;
            x[at] = B + (uint32_t)at;
            CHECK(sbq::beam_materials(x.data(), x.size(), beams.data(), B, mat) == sbq::BAD_BEAM_SLOT);
            defects++;
        }
    }
    // more caller slots than the engine has, through the identity
    {
        g_what = "identity past B";
        std::vector<float> mat;
        CHECK(sbq::beam_materials(nullptr, B, beams.data(), B - 1u, mat) == sbq::BAD_BEAM_SLOT);
        defects++;
    }
    printf("FORCES_TABLES_OK %u particles %u beams %d defects\n", P, B, defects);
    return 0;
}
