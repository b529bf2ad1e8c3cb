// blocked_word_check.cpp -- csrc/sb_blocked_word.h on the CPU: the entry word as k_substep_blocked holds it (wide as in HBM,
// or repacked narrow into byte offsets) and the LDS planes those offsets address.
//   usage: blocked_word_check          prints BLOCKED_WORD_OK, or the first mismatch and exits 1
#include <cstdio>
#include <cstdlib>
#include <set>

#include "sb_blocked_word.h"

static int fail(const char *what, uint32_t a, uint32_t b, uint32_t row, uint32_t got, uint32_t want)
{
    std::printf("MISMATCH %s: A=%u B=%u row=%u got %u want %u\n", what, a, b, row, got, want);
    return 1;
}

template <bool NARROW> static int check_word(uint32_t w, uint32_t a, uint32_t b, uint32_t row)
{
    const char *form = NARROW ? "narrow" : "wide";
    if (sbw::a4<NARROW>(w) != 4u * a) return fail(form, a, b, row, sbw::a4<NARROW>(w), 4u * a);
    if (sbw::b4<NARROW>(w) != 4u * b) return fail(form, a, b, row, sbw::b4<NARROW>(w), 4u * b);
    if (sbw::row<NARROW>(w) != row) return fail(form, a, b, row, sbw::row<NARROW>(w), row);
    if (sbw::row32<NARROW>(w) != 32u * row) return fail(form, a, b, row, sbw::row32<NARROW>(w), 32u * row);
    return 0;
}

int main()
{
    // region indices: the first records, both sides of bit 10, the last region particle (2559), the two dummy records (2560, 2561),
    // the first and the last padding record (2562, 2689)
    const uint32_t idx[] = {0u, 1u, 1023u, 1024u, 2559u, 2560u, 2561u, 2562u, 2689u};
    std::set<uint32_t> narrow_seen;
    for (uint32_t a : idx)
        for (uint32_t b : idx) {
            for (uint32_t row = 0; row < SBW_NARROW_ROWS; row++) {
                const uint32_t wide = sbw::pack_wide(a, b, row), narrow = sbw::repack(wide);
                if (narrow != sbw::pack_narrow(a, b, row)) return fail("repack", a, b, row, narrow, sbw::pack_narrow(a, b, row));
                if (sbw::held<true>(wide) != narrow || sbw::held<false>(wide) != wide) return fail("held", a, b, row, sbw::held<true>(wide), narrow);
                if (check_word<true>(narrow, a, b, row) || check_word<false>(wide, a, b, row)) return 1;
                if ((narrow & 3u) || ((narrow >> 14) & 3u)) return fail("narrow: low bits of a field", a, b, row, narrow, 0u);
                if (!narrow_seen.insert(narrow).second) return fail("repack is not one to one", a, b, row, narrow, 0u);
            }
            for (uint32_t row : {16u, 17u, 255u}) // more rows than a narrow word names: the wide word stays
                if (check_word<false>(sbw::pack_wide(a, b, row), a, b, row)) return 1;
        }
    // a dead entry still reads as dead after the repack, and as nothing else: the dummy word is (2560, 2561, row 0)
    const uint32_t dummy = sbw::pack_wide(2560u, 2561u, 0u);
    for (uint32_t a : idx)
        for (uint32_t b : idx)
            for (uint32_t row = 0; row < SBW_NARROW_ROWS; row++)
                if ((sbw::repack(sbw::pack_wide(a, b, row)) == sbw::repack(dummy)) != (a == 2560u && b == 2561u && row == 0u))
                    return fail("dummy", a, b, row, 0u, 0u);
    // planes: four of them, disjoint for every record, each a whole number of 64-dword steps from the first, all of it inside the
    // offsets a DS instruction carries
    for (uint32_t pl = 0; pl < 4u; pl++) {
        if (sbw::plane_bytes(pl) != 4u * SBW_PLANE * pl) return fail("plane offset", pl, 0u, 0u, sbw::plane_bytes(pl), 4u * SBW_PLANE * pl);
        if (sbw::plane_bytes(pl) % 256u) return fail("plane offset is not a multiple of 64 dwords", pl, 0u, 0u, sbw::plane_bytes(pl), 0u);
        if (sbw::plane_bytes(pl) / 256u > 255u || sbw::plane_bytes(pl) > 65535u) return fail("plane offset does not fit", pl, 0u, 0u, sbw::plane_bytes(pl), 0u);
        if (pl && 4u * (SBW_CAP - 1u) + sbw::plane_bytes(pl - 1u) >= sbw::plane_bytes(pl)) return fail("planes overlap", pl, 0u, 0u, 0u, 0u);
    }
    if (sbw::plane_bytes(SBW_PY) / 256u != 43u || sbw::plane_bytes(SBW_FX) != 22016u || sbw::plane_bytes(SBW_FY) != 33024u)
        return fail("plane constants", 0u, 0u, 0u, sbw::plane_bytes(SBW_FY), 33024u);
    std::printf("BLOCKED_WORD_OK\n");
    return 0;
}
