// batch_ray_check.cpp -- csrc/sb_batch_ray_math.h on the host (`make hostcheck`, under AddressSanitizer + UBSan and under
// ThreadSanitizer): the rows of a ray cast against the particles, beams and walls of scenes read from a file, printed one line per
// row for tests/test_batch_raycast_cpu.py to compare with tests/batch_raycast_ref.py bit for bit.  Stand-alone: nothing here is
// loaded into Python.
//
// The file is little-endian words, scene after scene: {P, B, k, labels (0 / 1), bounds, radius} (the last two float bits), then P
// particles {data index, x, y, label}, B beams {data index, ax, ay, bx, by, label of endpoint A}, k rows of 8 words.  Output per
// row: "<t bits, hex> <kind> <index>".  The primitives are walked backwards and in two halves that are combined at the end: the
// winner is an integer minimum, so the order cannot show.
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "sb_batch_ray_math.h"

struct Scene {
    uint32_t P, B, k, labels;
    float bounds, radius;
    const uint32_t *part, *beam, *rows;
};

static uint64_t walk(const Scene &s, const sbr::Ray &r, uint32_t half)
{
    const float r2 = s.radius * s.radius;
    uint64_t key = SBR_NO_KEY;
    if (r.mask & sbr::MASK_PARTICLES)
        for (uint32_t i = s.P; i-- > 0u;) {
            const uint32_t *p = s.part + 4u * i;
            if ((i & 1u) != half || sbr::skipped(r, (int32_t)p[3])) continue;
            key = sbr::nearer(key, sbr::disc(r, sbr::word_as_float(p[1]), sbr::word_as_float(p[2]), r2, p[0]));
        }
    if (r.mask & sbr::MASK_BEAMS)
        for (uint32_t j = s.B; j-- > 0u;) {
            const uint32_t *b = s.beam + 6u * j;
            if ((j & 1u) != half || sbr::skipped(r, (int32_t)b[5])) continue;
            key = sbr::nearer(key, sbr::segment(r, sbr::word_as_float(b[1]), sbr::word_as_float(b[2]), sbr::word_as_float(b[3]), sbr::word_as_float(b[4]), b[0]));
        }
    if ((r.mask & sbr::MASK_WALLS) && half == 0u) key = sbr::nearer(key, sbr::walls(r, s.bounds));
    return key;
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
    while (at + 6u <= words.size()) {
        Scene s{words[at], words[at + 1], words[at + 2], words[at + 3], sbr::word_as_float(words[at + 4]), sbr::word_as_float(words[at + 5]), nullptr, nullptr, nullptr};
        const size_t need = 4u * (size_t)s.P + 6u * (size_t)s.B + (size_t)SBR_ROW_WORDS * s.k;
        if (at + 6u + need > words.size()) {
            fprintf(stderr, "scene %zu is cut short\n", scenes.size());
            return 2;
        }
        s.part = words.data() + at + 6u, s.beam = s.part + 4u * (size_t)s.P, s.rows = s.beam + 6u * (size_t)s.B;
        scenes.push_back(s);
        at += 6u + need, rows += s.k;
    }
    struct Out {
        uint32_t t;
        int32_t kind, index;
    };
    std::vector<std::vector<Out>> out(scenes.size());
    // two threads over the scenes, even and odd: the header keeps no state, which ThreadSanitizer confirms
    auto run = [&](size_t first) {
        for (size_t i = first; i < scenes.size(); i += 2) {
            const Scene &s = scenes[i];
            out[i].resize(s.k);
            for (uint32_t j = 0; j < s.k; j++) {
                const uint32_t *row = s.rows + (size_t)SBR_ROW_WORDS * j;
                const int v = sbr::row_verdict(row, s.labels != 0u);
                uint64_t key = SBR_NO_KEY;
                if (v == sbr::MISS) {
                    const sbr::Ray r = sbr::ray_of(row);
                    key = sbr::nearer(walk(s, r, 1u), walk(s, r, 0u));
                }
                out[i][j] = Out{sbr::out_t(v, key, row[5]), sbr::out_kind(v, key), sbr::out_index(v, key)};
            }
        }
    };
    std::thread t0(run, 0), t1(run, 1);
    t0.join();
    t1.join();
    for (const auto &scene : out)
        for (const Out &o : scene) printf("%08x %d %d\n", o.t, o.kind, o.index);
    printf("BATCH_RAY_CHECK_OK %zu %zu\n", scenes.size(), rows);
    return 0;
}
