// Host-only count of what the beam phase of k_substep_blocked evaluates against what its substeps need, from the plan
// alone (softbody-webgpu_amd/csrc/sb_blocking.h); plain g++, no HIP:
//   g++ -O2 -std=c++17 -pthread -Isoftbody-webgpu_amd/csrc tools/blocked_prefix_waste.cpp -o blocked_prefix_waste
//   usage: blocked_prefix_waste <width> <height> <target> <K> [k_run ...]      (default k_run: K)
// The scene is bench.py's lattice (scenes.lattice_buffers: spacing 30, origin 1000, jitter 1.0, seed 1, three beams per
// particle); BASELINE config 2 on a 256-CU device is `1000 1000 977 7 6 7` (sb_api.hip upload_plan: 977 particles per tile,
// plan depth SB_BK_KPLAN = 7, long calls run launches of 6).
// Every thread's group test is replayed per tile and substep under two slot -> entry mappings:
//   strided   slot i of thread tid holds entry base + tid + i T                        (the kernel's until this tool was written)
//   paired    group g = i / 2 of wave w, lane l holds entries base + g 2T + 128 w + l + 64 (i & 1)     (the kernel's: SB_ENT_L)
// (base = 0 for own slots, n_ownb for halo slots; T = 512 threads, groups of G = 2 slots; a group runs when its FIRST entry is
// inside the substep's prefix -- n_ownb for own slots, lvl_cnt[k_run - s] for halo slots).  Counted per mapping, summed over
// tiles and the substeps of one launch: entries evaluated, entries needed, real entries past the prefix, padding entries
// (slots with no entry behind them), thread groups skipped, and the wave-groups that issue instructions (a wave runs a group's
// code when any of its 64 lanes does: that is what the VALU instruction count of the beam phase follows).
// The paired mapping is also CHECKED: every needed entry is evaluated exactly once per substep, and no thread group holds
// more than one entry past its class's prefix.  Exit status 1 if not.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sb_blocking.h"

static const uint32_t T = 512, G = 2, OWNB = 6, MAXB = 12, WAVE = 64;

static double hash_uniform(uint64_t seed, uint64_t i)
{ // scenes.hash_uniform: splitmix64 of (seed * 2^32 + i) -> [-1, 1)
    uint64_t x = (seed << 32) + i;
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return (double)(x >> 11) / 4503599627370496.0 - 1.0;
}

struct Counts {
    uint64_t evaluated = 0, needed = 0, past = 0, padding = 0, groups_run = 0, groups_skipped = 0, wave_groups = 0, missed = 0, twice = 0,
             wide = 0;
};

// the entry (list index within the tile) behind slot i of thread tid; own slots count from 0, halo slots from n_ownb
static uint32_t entry_of(bool paired, uint32_t tid, uint32_t i, uint32_t n_ownb)
{
    const bool own = i < OWNB;
    const uint32_t base = own ? 0u : n_ownb, il = own ? i : i - OWNB;
    return paired ? base + (il / G) * (G * T) + tid + (tid & ~(WAVE - 1u)) + (il % G) * WAVE : base + tid + il * T;
}

int main(int argc, char **argv)
{
    if (argc < 5) {
        fprintf(stderr, "usage: %s <width> <height> <target> <K> [k_run ...]\n", argv[0]);
        return 2;
    }
    const uint32_t w = atoi(argv[1]), h = atoi(argv[2]), target = atoi(argv[3]), K = atoi(argv[4]);
    std::vector<uint32_t> runs;
    for (int a = 5; a < argc; a++) runs.push_back(atoi(argv[a]));
    if (runs.empty()) runs.push_back(K);
    const uint32_t P = w * h;
    std::vector<float> px(P), py(P);
    SbHostBeams beams;
    auto add = [&](uint32_t a, uint32_t b) { SbHostBeam s{}; s.a = a; s.b = b; beams.push_back(s); };
    for (uint32_t x = 0; x < w; x++)
        for (uint32_t y = 0; y < h; y++) {
            const uint32_t i = x * h + y;
            px[i] = (float)(x * 30.0 + 1000.0) + (float)hash_uniform(1, 2ull * i);
            py[i] = (float)(y * 30.0 + 1000.0) + (float)hash_uniform(1, 2ull * i + 1);
            if (y + 1 < h) add(i, i + 1);
            if (x + 1 < w) add(i, i + h);
            if (y + 1 < h && x + 1 < w) add(i, i + h + 1);
        }
    SbBlocking t;
    sb_build_blocking(t, px, py, beams, target, K);
    printf("scene %u x %u lattice, %u particles, %zu beams; tile target %u -> %u tiles, plan depth K = %u\n", w, h, P, beams.size(), target,
           t.ntiles, K);
    printf("largest tile: %u own particles, %u own beams, %u entries\n", t.max_own, t.max_ownb, t.max_entries);
    if (t.max_ownb > OWNB * T) {
        fprintf(stderr, "a tile owns %u beams: more than the kernel's %u own slots\n", t.max_ownb, OWNB * T);
        return 2;
    }
    bool ok = true;
    for (uint32_t k_run : runs) {
        if (k_run < 1 || k_run > K || t.halo_entries_at[k_run] > (MAXB - OWNB) * T) {
            fprintf(stderr, "k_run %u: outside the plan, or more halo entries than the kernel's slots\n", k_run);
            return 2;
        }
        Counts c[2];
        std::vector<uint8_t> hits;
        for (uint32_t k = 0; k < t.ntiles; k++) {
            const uint32_t *lc = &t.lvl_cnt[(size_t)k * K];
            const uint32_t n_ownb = t.tile_b0[k + 1] - t.tile_b0[k], ne_load = lc[k_run - 1];
            for (uint32_t s = 1; s <= k_run; s++) {
                const uint32_t nbl = lc[k_run - s]; // (counts the own entries too)
                for (int paired = 0; paired < 2; paired++) {
                    Counts &n = c[paired];
                    n.needed += nbl;
                    hits.assign(std::max(nbl, 1u), 0);
                    for (uint32_t i0 = 0; i0 < MAXB; i0 += G)
                        for (uint32_t wv = 0; wv < T / WAVE; wv++) {
                            bool wave_runs = false;
                            for (uint32_t tid = wv * WAVE; tid < (wv + 1) * WAVE; tid++) {
                                const bool own = i0 < OWNB;
                                const uint32_t limit = own ? n_ownb : nbl, have = own ? n_ownb : ne_load;
                                if (!(entry_of(paired, tid, i0, n_ownb) < limit)) {
                                    n.groups_skipped++;
                                    continue;
                                }
                                wave_runs = true;
                                n.groups_run++;
                                uint32_t beyond = 0;
                                for (uint32_t u = 0; u < G; u++) {
                                    const uint32_t j = entry_of(paired, tid, i0 + u, n_ownb);
                                    n.evaluated++;
                                    if (j < limit) {
                                        if (hits[j]++) n.twice++;
                                    } else {
                                        beyond++;
                                        if (j < have) n.past++;
                                        else n.padding++;
                                    }
                                }
                                if (beyond > 1) n.wide++;
                            }
                            n.wave_groups += wave_runs;
                        }
                    for (uint32_t j = 0; j < nbl; j++) n.missed += hits[j] == 0;
                }
            }
        }
        printf("\nk_run = %u (one launch: %u tiles x %u substeps)\n", k_run, t.ntiles, k_run);
        printf("%-8s %14s %14s %12s %12s %8s %14s %14s %12s\n", "mapping", "evaluated", "needed", "past prefix", "padding", "waste %", "groups run",
               "groups skipped", "wave-groups");
        for (int paired = 0; paired < 2; paired++) {
            const Counts &n = c[paired];
            printf("%-8s %14llu %14llu %12llu %12llu %8.2f %14llu %14llu %12llu\n", paired ? "paired" : "strided", (unsigned long long)n.evaluated,
                   (unsigned long long)n.needed, (unsigned long long)n.past, (unsigned long long)n.padding,
                   100.0 * (double)(n.evaluated - n.needed) / (double)n.evaluated, (unsigned long long)n.groups_run,
                   (unsigned long long)n.groups_skipped, (unsigned long long)n.wave_groups);
            if (n.missed || n.twice) {
                printf("  %s: %llu needed entries not evaluated, %llu evaluated twice\n", paired ? "paired" : "strided", (unsigned long long)n.missed,
                       (unsigned long long)n.twice);
                ok = false;
            }
        }
        printf("per tile and substep: strided %.1f entries in %.2f wave-groups, paired %.1f in %.2f, needed %.1f\n",
               (double)c[0].evaluated / (t.ntiles * k_run), (double)c[0].wave_groups / (t.ntiles * k_run), (double)c[1].evaluated / (t.ntiles * k_run),
               (double)c[1].wave_groups / (t.ntiles * k_run), (double)c[0].needed / (t.ntiles * k_run));
        printf("paired / strided: entries %.4f, wave-groups %.4f\n", (double)c[1].evaluated / (double)c[0].evaluated,
               (double)c[1].wave_groups / (double)c[0].wave_groups);
        if (c[1].wide) {
            printf("  paired: %llu thread groups hold more than one entry past the prefix\n", (unsigned long long)c[1].wide);
            ok = false;
        }
    }
    printf(ok ? "\nPREFIX_WASTE_OK\n" : "\nPREFIX_WASTE_FAILED\n");
    return ok ? 0 : 1;
}
