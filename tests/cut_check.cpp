// cut_check.cpp -- check driver of csrc/sb_cut_math.h on the host (built by `make hostcheck`, once under AddressSanitizer + UBSan and
// once under ThreadSanitizer, with -ffp-contract=off as the library is).  Reads a file of records of 12 words -- a shape (8 words),
// A.x, A.y, B.x, B.y -- and writes one character per record to stdout: '1' hit, '0' not.  tests/test_cut_cpu.py compares the
// answers with tests/cut_ref.py.
#include <cstdio>
#include <vector>

#include "sb_cut_math.h"

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s <records>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    std::vector<uint32_t> rec(12);
    std::vector<char> out;
    while (fread(rec.data(), 4, 12, f) == 12) {
        const sbx::Shape s = sbx::shape_of(rec.data());
        const sbx::P2 A{sbx::word_as_float(rec[8]), sbx::word_as_float(rec[9])}, B{sbx::word_as_float(rec[10]), sbx::word_as_float(rec[11])};
        out.push_back(sbx::shape_hits(s, A, B) ? '1' : '0');
    }
    fclose(f);
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
