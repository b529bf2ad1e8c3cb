// batch_alloc_check.cpp -- csrc/sb_batch_alloc.h on the host (`make hostcheck`, under AddressSanitizer + UBSan and under
// ThreadSanitizer): the free bitmap of occupancy bytes read from a file of records and every r-th free index of it, printed one
// line per record for tests/test_batch_alloc_cpu.py to compare with numpy.  Stand-alone: nothing here is loaded into Python.
//
// A record is three little-endian words {capacity, loaded, rows (1 or 2)}, then per row the capacity rounded up to a multiple of
// four in occupancy bytes (the bytes past the capacity are padding: whatever the file holds there).  Each row is copied into a
// heap block of exactly that size, so a read past the padding is AddressSanitizer's to report.
// Output per record: the bitmap words in hex, " |", then the r-th free index for r = 0 .. free count - 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "sb_batch_alloc.h"

struct Record {
    uint32_t capacity, loaded;
    std::vector<uint32_t> occ, occ_b; // occ_b empty: one row
};

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
    std::vector<Record> rec;
    uint32_t head[3];
    while (fread(head, sizeof head, 1, f) == 1) {
        Record r{head[0], head[1], {}, {}};
        const size_t words = (r.capacity + 3u) / 4u;
        if (r.capacity == 0u || (head[2] != 1u && head[2] != 2u)) {
            fprintf(stderr, "record %zu: capacity %u, %u rows\n", rec.size(), head[0], head[2]);
            return 2;
        }
        r.occ.resize(words);
        if (fread(r.occ.data(), 4, words, f) != words) return 2;
        if (head[2] == 2u) {
            r.occ_b.resize(words);
            if (fread(r.occ_b.data(), 4, words, f) != words) return 2;
        }
        rec.push_back(std::move(r));
    }
    fclose(f);
    const size_t n = rec.size();
    std::vector<std::string> line(n);
    // two threads over disjoint halves: the header keeps no state, which ThreadSanitizer confirms
    auto run = [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            const Record &r = rec[i];
            const uint32_t nw = sba::bitmap_words(r.capacity);
            std::vector<uint32_t> bits(nw), prefix(nw + 1u);
            char text[16];
            for (uint32_t w = 0; w < nw; w++) {
                bits[w] = sba::free_word(r.occ.data(), r.occ_b.empty() ? nullptr : r.occ_b.data(), r.capacity, r.loaded != 0u, w);
                prefix[w + 1u] = prefix[w] + (uint32_t)__builtin_popcount(bits[w]);
                snprintf(text, sizeof text, "%s%08x", w ? " " : "", bits[w]);
                line[i] += text;
            }
            line[i] += " |";
            auto nth_free = [&](uint32_t k) {
                if (k >= prefix[nw]) abort(); // r at and past the free count is never asked of the routine: the caller's room test
                return sba::nth_free(bits.data(), prefix.data(), nw, k);
            };
            for (uint32_t k = 0; k < prefix[nw]; k++) {
                snprintf(text, sizeof text, " %u", nth_free(k));
                line[i] += text;
            }
        }
    };
    std::thread t0(run, 0, n / 2), t1(run, n / 2, n);
    t0.join();
    t1.join();
    for (size_t i = 0; i < n; i++) printf("%s\n", line[i].c_str());
    return 0;
}
