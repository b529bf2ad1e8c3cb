// batch_near_check.cpp -- csrc/sb_batch_near_math.h on the host (`make hostcheck`, under AddressSanitizer + UBSan and under
// ThreadSanitizer): the rows of a proximity query against the particles, beams and walls of scenes read from a file, printed one
// line per row for tests/test_batch_nearest_cpu.py to compare with tests/batch_nearest_ref.py bit for bit.  Stand-alone: nothing
// here is loaded into Python.
//
// The file is little-endian words, scene after scene: {P, B, k, labels (0 / 1), bounds (float bits)}, then P particles {data
// index, x, y, label}, B beams {data index, ax, ay, bx, by, label of endpoint A}, k rows of 8 words.  Output per row:
// "<d2 bits of the winner, hex> <kind> <index> <qx bits> <qy bits> <particles within> <beams within>" (d2 and Q are zeros where
// there is no winner).  The primitives are walked backwards and in two halves that are combined at the end: the winner is an
// integer minimum and the counts are sums, so the order cannot show.
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "sb_batch_near_math.h"

struct Scene {
    uint32_t P, B, k, labels;
    float bounds;
    const uint32_t *part, *beam, *rows;
};

static uint64_t walk(const Scene &s, const sbn::Probe &q, uint32_t half, uint32_t *in_p, uint32_t *in_b)
{
    uint64_t key = SBN_NO_KEY;
    if (q.mask & sbn::MASK_PARTICLES)
        for (uint32_t i = s.P; i-- > 0u;) {
            const uint32_t *p = s.part + 4u * i;
            if ((i & 1u) != half || sbn::skipped(q, (int32_t)p[3])) continue;
            const uint64_t cand = sbn::particle(q, sbn::word_as_float(p[1]), sbn::word_as_float(p[2]), p[0]);
            *in_p += cand != SBN_NO_KEY;
            key = sbn::nearer(key, cand);
        }
    if (q.mask & sbn::MASK_BEAMS)
        for (uint32_t j = s.B; j-- > 0u;) {
            const uint32_t *b = s.beam + 6u * j;
            if ((j & 1u) != half || sbn::skipped(q, (int32_t)b[5])) continue;
            const uint64_t cand = sbn::segment(q, sbn::word_as_float(b[1]), sbn::word_as_float(b[2]), sbn::word_as_float(b[3]), sbn::word_as_float(b[4]), b[0]);
            *in_b += cand != SBN_NO_KEY;
            key = sbn::nearer(key, cand);
        }
    if ((q.mask & sbn::MASK_WALLS) && half == 0u) key = sbn::nearer(key, sbn::walls(q, s.bounds));
    return key;
}

// the winner's closest point, computed again from the winner (the kernel looks the primitive up by its data index; here: a search)
static void closest(const Scene &s, const sbn::Probe &q, uint64_t key, float *qx, float *qy)
{
    const uint32_t kind = sbn::key_kind(key), index = sbn::key_index(key);
    if (kind == sbn::PARTICLE) {
        for (uint32_t i = 0; i < s.P; i++)
            if (s.part[4u * i] == index) *qx = sbn::word_as_float(s.part[4u * i + 1u]), *qy = sbn::word_as_float(s.part[4u * i + 2u]);
    } else if (kind == sbn::BEAM) {
        for (uint32_t j = 0; j < s.B; j++) {
            const uint32_t *b = s.beam + 6u * j;
            if (b[0] == index) sbn::segment_q(q, sbn::word_as_float(b[1]), sbn::word_as_float(b[2]), sbn::word_as_float(b[3]), sbn::word_as_float(b[4]), qx, qy);
        }
    } else {
        sbn::wall_q(q, s.bounds, index, qx, qy);
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s scenes.bin\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    std::vector<uint32_t> words;
    uint32_t w;
    while (fread(&w, sizeof w, 1, f) == 1) words.push_back(w);
    fclose(f);
    std::vector<Scene> scenes;
    size_t at = 0, rows = 0;
    while (at + 5u <= words.size()) {
        Scene s{words[at], words[at + 1], words[at + 2], words[at + 3], sbn::word_as_float(words[at + 4]), nullptr, nullptr, nullptr};
        const size_t need = 4u * (size_t)s.P + 6u * (size_t)s.B + (size_t)SBN_ROW_WORDS * s.k;
        if (at + 5u + need > words.size()) {
            fprintf(stderr, "scene %zu is cut short\n", scenes.size());
            return 2;
        }
        s.part = words.data() + at + 5u, s.beam = s.part + 4u * (size_t)s.P, s.rows = s.beam + 6u * (size_t)s.B;
        scenes.push_back(s);
        at += 5u + need, rows += s.k;
    }
    struct Out {
        uint32_t d2;
        int32_t kind, index;
        uint32_t qx, qy, in_p, in_b;
    };
    std::vector<std::vector<Out>> out(scenes.size());
    // two threads over the scenes, even and odd: the header keeps no state, which ThreadSanitizer confirms
    auto run = [&](size_t first) {
        for (size_t i = first; i < scenes.size(); i += 2) {
            const Scene &s = scenes[i];
            out[i].resize(s.k);
            for (uint32_t j = 0; j < s.k; j++) {
                const uint32_t *row = s.rows + (size_t)SBN_ROW_WORDS * j;
                const int v = sbn::row_verdict(row, s.labels != 0u);
                uint64_t key = SBN_NO_KEY;
                uint32_t in_p = 0u, in_b = 0u;
                float qx = 0.0f, qy = 0.0f;
                if (v == sbn::MISS) {
                    const sbn::Probe q = sbn::probe_of(row);
                    key = walk(s, q, 1u, &in_p, &in_b);
                    key = sbn::nearer(key, walk(s, q, 0u, &in_p, &in_b));
                    if (key != SBN_NO_KEY) closest(s, q, key, &qx, &qy);
                }
                out[i][j] = Out{key == SBN_NO_KEY ? 0u : sbn::key_d2(key), sbn::out_kind(v, key), sbn::out_index(v, key), sbn::float_as_word(qx),
                                sbn::float_as_word(qy), in_p, in_b};
            }
        }
    };
    std::thread t0(run, 0), t1(run, 1);
    t0.join();
    t1.join();
    for (const auto &scene : out)
        for (const Out &o : scene) printf("%08x %d %d %08x %08x %u %u\n", o.d2, o.kind, o.index, o.qx, o.qy, o.in_p, o.in_b);
    printf("BATCH_NEAR_CHECK_OK %zu %zu\n", scenes.size(), rows);
    return 0;
}
