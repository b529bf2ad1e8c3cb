// batch_forces_check.cpp -- csrc/sb_batch_forces_math.h on the host (`make hostcheck`, under AddressSanitizer + UBSan and under
// ThreadSanitizer, with -ffp-contract=off): a beam's force_mag and the contact sums of a particle, on records that
// tests/test_batch_forces_cpu.py writes and whose results it compares, bit for bit, with tests/batch_forces_ref.py.
//
// Input (little endian, 32-bit words), records until the end of the file:
//   1, then 8 floats {ax, ay, bx, by, target_length, last_length, spring, damp}                 -> "b <force_mag bits>"
//   2, n, 5 floats {two_r, friction, elasticity_coeff, inv_dt2, dt2}, then n x 5 floats {dx, dy, dist, ux, uy}, the partners of
//      one particle in the order they are applied                                                -> "c <push_x> <push_y> <impulse_x>
//                                                                                                   <impulse_y> <depth> <partners>"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sb_batch_forces_math.h"

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint32_t> w;
    uint32_t buf[1024];
    size_t n;
    while ((n = fread(buf, 4, 1024, f)) > 0) w.insert(w.end(), buf, buf + n);
    fclose(f);
    size_t at = 0;
    auto flt = [&](size_t i) {
        float v;
        memcpy(&v, &w.at(i), 4);
        return v;
    };
    while (at < w.size()) {
        const uint32_t kind = w.at(at++);
        if (kind == 1u) {
            if (at + 8 > w.size()) return 3;
            printf("b %08x\n", bits(sbf_force_mag(flt(at), flt(at + 1), flt(at + 2), flt(at + 3), flt(at + 4), flt(at + 5), flt(at + 6), flt(at + 7))));
            at += 8;
        } else if (kind == 2u) {
            if (at + 6 > w.size()) return 3;
            const uint32_t partners = w.at(at);
            const float two_r = flt(at + 1), friction = flt(at + 2), ecoef = flt(at + 3), inv_dt2 = flt(at + 4), dt2 = flt(at + 5);
            at += 6;
            if (at + 5 * (size_t)partners > w.size()) return 3;
            SbfContact c = sbf_contact_zero();
            for (uint32_t k = 0; k < partners; k++, at += 5) {
                if (!sbf_is_partner(flt(at + 2), two_r)) return 4;
                sbf_contact_add(c, flt(at), flt(at + 1), flt(at + 2), flt(at + 3), flt(at + 4), two_r, friction, ecoef, inv_dt2, dt2);
            }
            printf("c %08x %08x %08x %08x %08x %u\n", bits(c.push_x), bits(c.push_y), bits(c.impulse_x), bits(c.impulse_y), bits(c.depth), c.partners);
        } else {
            return 3;
        }
    }
    return 0;
}
