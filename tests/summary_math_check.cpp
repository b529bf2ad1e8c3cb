// summary_math_check.cpp -- check driver of csrc/sb_summary_math.h on the host (built by `make hostcheck`, once under AddressSanitizer +
// UBSan and once under ThreadSanitizer, with -ffp-contract=off as the library is).  Reads one scene -- six words {max_particles,
// max_beams, particles, live beams, removed beams, pending breaks}, then per particle {data index, x, y, vx, vy, ax, ay}, then per
// live beam {data index, strain, stress} -- and writes the 24 words of its scene row in hex: the header's leaves, the header's tree
// over all W leaves, the header's row former.  tests/test_batch_summary_cpu.py compares them with tests/batch_summary_ref.py.
#include <cstdio>
#include <vector>

#include "sb_summary_math.h"

static const uint32_t MAX_W = 4096u;

struct Scene {
    std::vector<uint32_t> rec;
    std::vector<int32_t> at; // data index -> record, -1: none
    uint32_t words;          // per record
};
struct ParticleLeaf {
    const Scene &s;
    SbuLocal &l;
    void operator()(uint32_t d, double (&out)[5]) const
    {
        for (int c = 0; c < 5; c++) out[c] = 0.0;
        if (s.at[d] < 0) return;
        const uint32_t *r = &s.rec[(size_t)s.at[d] * s.words];
        sbu_local_particle(l, sbu_float2{sbu_float(r[1]), sbu_float(r[2])}, sbu_float2{sbu_float(r[3]), sbu_float(r[4])},
                           sbu_float2{sbu_float(r[5]), sbu_float(r[6])}, out);
    }
};
struct BeamLeaf {
    const Scene &s;
    SbuLocal &l;
    void operator()(uint32_t d, double (&out)[1]) const
    {
        out[0] = 0.0;
        if (s.at[d] < 0) return;
        const uint32_t *r = &s.rec[(size_t)s.at[d] * s.words];
        sbu_local_beam(l, sbu_float(r[1]), sbu_float(r[2]), out);
    }
};

// sbu_tree<W> for the W of the scene
template <uint32_t W, int N, class Leaf>
static bool tree_of(uint32_t w, const Leaf &leaf, double (&out)[N])
{
    if (w == W) {
        sbu_tree<(int)W, N>(leaf, 0u, 1u, out);
        return true;
    }
    if constexpr (W > 1u) return tree_of<W / 2u, N>(w, leaf, out);
    return false;
}

static bool read_scene(FILE *f, uint32_t n, uint32_t words, uint32_t W, Scene &s)
{
    s.words = words;
    s.rec.resize((size_t)n * words);
    s.at.assign(W, -1);
    if (n && fread(s.rec.data(), 4, s.rec.size(), f) != s.rec.size()) return false;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t d = s.rec[(size_t)i * words];
        if (d >= W || s.at[d] >= 0) return false;
        s.at[d] = (int32_t)i;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s <scene>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    uint32_t hd[6];
    Scene ps, bs;
    bool ok = fread(hd, 4, 6, f) == 6 && hd[0] <= MAX_W && hd[1] <= MAX_W && hd[2] <= hd[0] && hd[3] <= hd[1];
    const uint32_t Wp = ok ? sbb_pow2_at_least(hd[0]) : 1u, Wb = ok ? sbb_pow2_at_least(hd[1]) : 1u;
    ok = ok && read_scene(f, hd[2], 7u, Wp, ps) && read_scene(f, hd[3], 3u, Wb, bs);
    fclose(f);
    SbuLocal l;
    double tot[5], strain[1];
    if (!ok || !tree_of<MAX_W>(Wp, ParticleLeaf{ps, l}, tot) || !tree_of<MAX_W>(Wb, BeamLeaf{bs, l}, strain)) {
        fprintf(stderr, "%s: not a scene of at most %u / %u\n", argv[1], MAX_W, MAX_W);
        return 2;
    }
    float row[24] = {(float)hd[2], (float)hd[3], (float)hd[4], (float)hd[5], (float)l.p_bad, (float)l.b_bad};
    sbu_row_sums(row, l.p_fin, tot);
    sbu_row_extremes(row, l.p_fin, l.b_fin, SbuRowKeys{l.minx, l.miny, l.maxx, l.maxy, (float)l.max_v2, l.max_strain, l.max_stress, l.min_stress});
    row[19] = l.b_fin ? (float)(strain[0] / (double)l.b_fin) : sbu_float(SBB_QNAN);
    row[20] = 1.0f;
    for (int w = 0; w < 24; w++) printf("%08x%c", sbu_bits(row[w]), w == 23 ? '\n' : ' ');
    return 0;
}
