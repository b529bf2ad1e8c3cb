// batch_add_check.cpp -- csrc/sb_batch_add_math.h on the host (`make hostcheck`, under AddressSanitizer + UBSan and under
// ThreadSanitizer): the verdict of new-beam rows read from a file of records, printed one line per record for
// tests/test_batch_add_beams_cpu.py to compare with tests/batch_add_beams_ref.py.  Stand-alone: nothing here is loaded into Python.
//
// A record is 17 little-endian words: the row's 8 words, flags, max_particles, loaded, holds_a, holds_b, and the positions of
// the two endpoints ax, ay, bx, by as float bits.  Output per record: "<verdict> <resolved length bits> <current distance bits>".
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "sb_batch_add_math.h"

#define REC_WORDS 17u

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s records.bin\n", argv[0]);
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
    const size_t n = rec.size() / REC_WORDS;
    std::vector<int> verdict(n);
    std::vector<float> length(n), current(n);
    // two threads over disjoint halves: the header keeps no state, which ThreadSanitizer confirms
    auto run = [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            const uint32_t *r = &rec[i * REC_WORDS];
            current[i] = sbw::distance(sbw::word_as_float(r[13]), sbw::word_as_float(r[14]), sbw::word_as_float(r[15]), sbw::word_as_float(r[16]));
            verdict[i] = sbw::row_verdict(r, r[8], r[9], r[10] != 0u, r[11] != 0u, r[12] != 0u, current[i], &length[i]);
        }
    };
    std::thread t0(run, 0, n / 2), t1(run, n / 2, n);
    t0.join();
    t1.join();
    for (size_t i = 0; i < n; i++) {
        uint32_t lb, cb;
        memcpy(&lb, &length[i], 4);
        memcpy(&cb, &current[i], 4);
        printf("%d %u %u\n", verdict[i], lb, cb);
    }
    return 0;
}
