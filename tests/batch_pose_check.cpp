// batch_pose_check.cpp -- csrc/sb_batch_pose_math.h on the host (`make hostcheck`, under AddressSanitizer + UBSan and under
// ThreadSanitizer, with -ffp-contract=off): the eleven leaves of a matched particle, and the moments, words 4 .. 16 of the row and
// the moment words derived from eleven sums, on records that tests/test_batch_pose_cpu.py writes and whose results it compares,
// bit for bit, with tests/batch_pose_ref.py.
//
// Input (little endian, 64-bit words), records until the end of the file:
//   1, then 6 words holding the bits of the floats {x, y, vx, vy, X, Y} in their low halves    -> "l" and 11 x the bits of a double
//   2, then the bits of 11 doubles (the sums) and of the double n >= 1                            -> "f", 13 x the bits of a float
//                                                                                                  (words 4 .. 16), 8 x the bits of
//                                                                                                  a double (the moments)
//   3                                                                                            -> "u", the row words 4 .. 23 and
//                                                                                                  the 8 moments of n == 0
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sb_batch_pose_math.h"

static uint64_t bits64(double d)
{
    uint64_t u;
    memcpy(&u, &d, 8);
    return u;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint64_t> w;
    uint64_t buf[1024];
    size_t n;
    while ((n = fread(buf, 8, 1024, f)) > 0) w.insert(w.end(), buf, buf + n);
    fclose(f);
    size_t at = 0;
    while (at < w.size()) {
        const uint64_t kind = w.at(at++);
        if (kind == 1u) {
            if (at + 6 > w.size()) return 3;
            float v[6];
            for (int k = 0; k < 6; k++) v[k] = sbu_float((uint32_t)w.at(at + k));
            at += 6;
            double leaf[SBP_NSUM];
            if (!sbp_ref_finite(sbu_float2{v[4], v[5]})) return 4;
            sbp_leaves(sbu_float2{v[0], v[1]}, sbu_float2{v[2], v[3]}, sbu_float2{v[4], v[5]}, leaf);
            printf("l");
            for (uint32_t k = 0; k < SBP_NSUM; k++) printf(" %016" PRIx64, bits64(leaf[k]));
            printf("\n");
        } else if (kind == 2u) {
            if (at + SBP_NSUM + 1 > w.size()) return 3;
            double S[SBP_NSUM];
            for (uint32_t k = 0; k < SBP_NSUM; k++) S[k] = sbu_canon(sbp_double(w.at(at + k)));
            const double cnt = sbp_double(w.at(at + SBP_NSUM));
            at += SBP_NSUM + 1;
            const SbpFit fit = sbp_fit(S, cnt);
            float row[24] = {0};
            double m[8];
            sbp_row_fit(row, S, cnt, fit);
            sbp_moments(m, cnt, fit);
            printf("f");
            for (int k = 4; k <= 16; k++) printf(" %08x", sbu_bits(row[k]));
            for (int k = 0; k < 8; k++) printf(" %016" PRIx64, bits64(m[k]));
            printf("\n");
        } else if (kind == 3u) {
            printf("u");
            for (uint32_t k = 4; k < 24; k++) printf(" %08x", sbu_bits(sbp_unmatched_word(k)));
            for (uint32_t k = 0; k < 8; k++) printf(" %016" PRIx64, bits64(sbp_unmatched_moment(k)));
            printf("\n");
        } else {
            return 3;
        }
    }
    return 0;
}
