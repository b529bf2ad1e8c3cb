// The byte offsets the blocked kernel's buffer form hands to range-checked loads and stores (csrc/sb_blocked_addr.h), on the CPU:
// for randomly drawn tile tables, every slot of every thread of a workgroup, every slot class --
//   a slot that has an element:  offset == size * (base + j), below the descriptor's size, and the access ends inside it
//   a slot that has none:        offset at or above the descriptor's size, and offset + 8 does not wrap
// and, over all threads, the in-range slots of a class name each of the tile's elements exactly once.
// The draws put n_own, n_ownb, nhe and nh_load at 0, at 1, at the slot boundaries (multiples of 64 and of 512, one less and one
// more) and at capacity, with the tile as the LAST of its arrays (the last lane's offset is the last valid one) or somewhere inside.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "sb_blocked_addr.h"

static const uint32_t T = SBA_T, OWNP = SBA_OWNP, HALOP = 3, OWNB = SBA_OWNB, HALOB = 6; // (sb_engine.h SB_BK_HALOP, SB_BK_HALOB)
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static int fails = 0;
#define CHECK(c, ...)                                        \
    do {                                                     \
        if (!(c)) {                                          \
            if (fails++ < 20) printf("FAIL " __VA_ARGS__), printf("\n"); \
        }                                                    \
    } while (0)

// a count for a class of `slots` slots per thread: the edges first, then anything
static uint32_t draw_count(uint32_t slots, uint32_t round)
{
    const uint32_t cap = slots * T;
    const uint32_t edges[] = {0u, 1u, 63u, 64u, 65u, 127u, 128u, 129u, T - 1u, T, T + 1u, 2u * T - 1u, 2u * T, 2u * T + 1u, cap - 1u, cap};
    const uint32_t ne = sizeof(edges) / sizeof(edges[0]);
    const uint32_t v = round < ne ? edges[round] : rnd() % (cap + 1u);
    return v > cap ? cap : v;
}

struct Seen {
    std::vector<uint32_t> n;
    void reset(size_t count) { n.assign(count, 0u); }
};

// one slot against one descriptor of `bytes` bytes; base + [0, count) are the elements the class may name
static void check_slot(const char *what, sba::Slot s, uint32_t size, uint64_t bytes, uint32_t base, uint32_t count, Seen &seen)
{
    const uint32_t o = sba::off(s.have, s.idx, size);
    if (s.have) {
        CHECK(s.idx >= base && s.idx - base < count, "%s: index %u outside [%u, %u)", what, s.idx, base, base + count);
        CHECK((uint64_t)o == (uint64_t)size * s.idx, "%s: offset %u != %u * %u", what, o, size, s.idx);
        CHECK((uint64_t)o + size <= bytes, "%s: offset %u + %u past the descriptor's %llu bytes", what, o, size, (unsigned long long)bytes);
        if (s.idx >= base && s.idx - base < count) seen.n[s.idx - base]++;
    } else {
        CHECK((uint64_t)o >= bytes, "%s: out-of-range offset %u below the descriptor's %llu bytes", what, o, (unsigned long long)bytes);
        CHECK((uint64_t)o + 8u <= 0xFFFFFFFFull, "%s: out-of-range offset %u wraps within an 8-byte access", what, o);
    }
}
static void check_seen(const char *what, const Seen &seen)
{
    for (size_t i = 0; i < seen.n.size(); i++) CHECK(seen.n[i] == 1u, "%s: element %zu named %u times", what, i, seen.n[i]);
}

int main()
{
    CHECK(sba::fits(0) && sba::fits(SBA_OUT) && !sba::fits((uint64_t)SBA_OUT + 1u) && !sba::fits(1ull << 32), "sba::fits");
    Seen seen;
    for (uint32_t round = 0; round < 400u; round++) {
        // the tile tables of one tile: the four counts at their edges in turn (every pairing over the rounds), bases anywhere
        const uint32_t n_own = draw_count(OWNP, round % 20u), nh_load = draw_count(HALOP, (round / 3u) % 20u);
        const uint32_t n_ownb = draw_count(OWNB, (round / 2u) % 20u), nhe = draw_count(HALOB, (round / 5u) % 20u);
        const bool last = (round & 1u) == 0u; // the tile ends its arrays: nothing behind its last element
        // (a big base now and then: offsets near the top of the 32-bit range, arrays just short of 4 GiB)
        const bool big = round % 7u == 3u;
        auto base_for = [&](uint32_t count, uint32_t size) {
            const uint64_t room = ((uint64_t)SBA_OUT / size) - count; // most elements in front of the tile
            return (uint32_t)(big ? room - rnd() % 1000u : rnd() % 100000u);
        };
        auto bytes_for = [&](uint32_t base, uint32_t count, uint32_t size) {
            uint64_t b = ((uint64_t)base + count + (last ? 0u : 1u + rnd() % 5000u)) * size;
            return b > (uint64_t)SBA_OUT ? (uint64_t)SBA_OUT / size * size : b;
        };
        const uint32_t p0 = base_for(n_own, 8), h0 = base_for(nh_load, 4), b0 = base_for(n_ownb, 4), s0 = base_for(nhe, 4);
        const uint32_t ne = n_ownb + nhe, e0 = base_for(ne, 4);
        const uint64_t part_bytes = bytes_for(p0, n_own, 8), halo_bytes = bytes_for(h0, nh_load, 4), state_bytes = bytes_for(b0, n_ownb, 4),
                       sidx_bytes = bytes_for(s0, nhe, 4), ent_bytes = bytes_for(e0, ne, 4);
        CHECK(sba::fits(part_bytes) && sba::fits(halo_bytes) && sba::fits(state_bytes) && sba::fits(sidx_bytes) && sba::fits(ent_bytes), "the draw fits");

        seen.reset(n_own);
        for (uint32_t t = 0; t < T; t++)
            for (uint32_t i = 0; i < OWNP; i++) check_slot("own particle", sba::own_particle(t, i, p0, n_own), 8, part_bytes, p0, n_own, seen);
        check_seen("own particle", seen);

        seen.reset(nh_load);
        for (uint32_t t = 0; t < T; t++)
            for (uint32_t i = 0; i < HALOP; i++) check_slot("halo index", sba::halo_index(t, i, h0, nh_load), 4, halo_bytes, h0, nh_load, seen);
        check_seen("halo index", seen);

        seen.reset(n_ownb);
        for (uint32_t t = 0; t < T; t++)
            for (uint32_t i = 0; i < OWNB; i++) check_slot("own beam", sba::own_beam(t, i, b0, n_ownb), 4, state_bytes, b0, n_ownb, seen);
        check_seen("own beam", seen);

        seen.reset(nhe);
        for (uint32_t t = 0; t < T; t++)
            for (uint32_t i = 0; i < HALOB; i++) check_slot("halo state index", sba::halo_state(t, i, s0, nhe), 4, sidx_bytes, s0, nhe, seen);
        check_seen("halo state index", seen);

        seen.reset(ne);
        for (uint32_t t = 0; t < T; t++)
            for (uint32_t i = 0; i < OWNB + HALOB; i++) {
                const sba::Slot s = sba::entry(t, i, e0, n_ownb, nhe);
                check_slot("entry", s, 4, ent_bytes, e0, ne, seen);
                // an own slot names the entry of its own beam; a halo slot the entry behind the tile's own ones
                if (i < OWNB) {
                    const sba::Slot b = sba::own_beam(t, i, b0, n_ownb);
                    CHECK(s.have == b.have && (!s.have || s.idx - e0 == b.idx - b0), "entry / own beam disagree at thread %u slot %u", t, i);
                } else {
                    const sba::Slot h = sba::halo_state(t, i - OWNB, s0, nhe);
                    CHECK(s.have == h.have && (!s.have || s.idx - e0 - n_ownb == h.idx - s0), "entry / halo state disagree at thread %u slot %u", t, i);
                }
            }
        check_seen("entry", seen);

        // the gathers of the second round: an index read from the plan, 8 and 4 bytes an element, anywhere in its array
        for (uint32_t k = 0; k < 64u; k++) {
            const uint32_t P = 1u + rnd() % (big ? 0x1FFFFFFEu : 100000u), idx = k == 0u ? P - 1u : rnd() % P;
            const bool have = (rnd() & 1u) != 0u;
            const sba::Slot s{have, idx};
            const uint32_t o8 = sba::off(s.have, s.idx, 8), o4 = sba::off(s.have, s.idx, 4);
            if (have) {
                CHECK((uint64_t)o8 == 8ull * idx && (uint64_t)o8 + 8u <= 8ull * P, "gather of 8 bytes: offset %u for index %u of %u", o8, idx, P);
                CHECK((uint64_t)o4 == 4ull * idx && (uint64_t)o4 + 4u <= 4ull * P, "gather of 4 bytes: offset %u for index %u of %u", o4, idx, P);
            } else {
                CHECK((uint64_t)o8 >= 8ull * P && (uint64_t)o4 >= 4ull * P, "gather: out-of-range offsets %u %u inside %u elements", o8, o4, P);
            }
        }
    }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("BLOCKED_OFFSETS_OK\n");
    return 0;
}
