// batch_spawn_check.cpp -- csrc/sb_batch_spawn_math.h and the contact test of csrc/sb_contact_cells.h on the host (`make hostcheck`, under AddressSanitizer + UBSan and under
// ThreadSanitizer): the verdict of new-particle rows and the contact test of the blocked rule, read from a file of records and
// printed one line per record for tests/test_batch_add_particles_cpu.py to compare with tests/batch_add_particles_ref.py.
// Stand-alone: nothing here is loaded into Python.
//
// A record is 12 little-endian words: the row's 8 words, loaded, the radius and the position of another particle ox, oy as float
// bits.  Output per record: "<verdict> <row touches the other position: 0 / 1>".  Behind the records of one GROUP (a word count
// n in argv[2]: the file's first n records are the rows of one call, E(j) = their touch column) the blocked rule over the group
// is printed as one line of 0 / 1 per row.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "sb_batch_spawn_math.h"
#include "sb_contact_cells.h" // the contact test of the blocked rule

#define REC_WORDS 12u

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s records.bin group_rows\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    std::vector<uint32_t> rec;
    uint32_t w[REC_WORDS];
    while (fread(w, sizeof w, 1, f) == 1) rec.insert(rec.end(), w, w + REC_WORDS);
    fclose(f);
    const size_t n = rec.size() / REC_WORDS, group = std::min<size_t>((size_t)atoi(argv[2]), n);
    std::vector<int> verdict(n), touches(n);
    // two threads over disjoint halves: the header keeps no state, which ThreadSanitizer confirms
    auto run = [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            const uint32_t *r = &rec[i * REC_WORDS];
            const SbTouchTest t = sb_touch_test(sbs::word_as_float(r[9]));
            verdict[i] = sbs::row_verdict(r, r[8] != 0u);
            touches[i] = sb_touch_xy(sbs::word_as_float(r[1]), sbs::word_as_float(r[2]), sbs::word_as_float(r[10]), sbs::word_as_float(r[11]), t.thr, t.two_r);
        }
    };
    std::thread t0(run, 0, n / 2), t1(run, n / 2, n);
    t0.join();
    t1.join();
    for (size_t i = 0; i < n; i++) printf("%d %d\n", verdict[i], touches[i]);
    for (size_t j = 0; j < group; j++) {
        const uint32_t *rj = &rec[j * REC_WORDS];
        const SbTouchTest t = sb_touch_test(sbs::word_as_float(rj[9]));
        const bool e_j = verdict[j] == sbs::SBS_CANDIDATE && touches[j] != 0;
        const bool b = verdict[j] == sbs::SBS_CANDIDATE &&
                       sbs::blocked(
                           (uint32_t)j, e_j, [&](uint32_t i) { return verdict[i]; }, [&](uint32_t i) { return touches[i] != 0; },
                           [&](uint32_t i) {
                               const uint32_t *ri = &rec[i * REC_WORDS];
                               return sb_touch_xy(sbs::word_as_float(rj[1]), sbs::word_as_float(rj[2]), sbs::word_as_float(ri[1]), sbs::word_as_float(ri[2]), t.thr,
                                                  t.two_r);
                           });
        printf("%d%s", b ? 1 : 0, j + 1 == group ? "\n" : " ");
    }
    return 0;
}
