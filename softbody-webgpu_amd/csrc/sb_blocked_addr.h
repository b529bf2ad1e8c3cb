// sb_blocked_addr.h -- where the load and store phases of k_substep_blocked find a thread's slots in HBM: the byte offsets that go
// into range-checked buffer instructions (sb_blocked.hip SbMem<true>), and the element indices of the flat form (SbMem<false>).
//
// A slot of a thread either names an element of an array (HAVE: its index follows from the tile tables) or nothing.  The flat
// form sends the lanes with nothing to element 0 and discards what comes back.  The buffer form gives them SBA_OUT, an offset at
// or past the size of every descriptor the host lets through (sba::fits): the hardware's range check returns 0 for such a load
// and drops such a store, so a request stays unconditional, the have-test is all the address arithmetic a lane with nothing
// does, and no line of element 0 is touched.  SBA_OUT is not 0xFFFFFFFF: the widest access is 8 bytes, and offset + 8 must not
// wrap whatever width the range check is computed in.
// Host and device: tests/blocked_offsets_check.cpp checks the formulas on a CPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBA_HD __host__ __device__ __forceinline__
#else
#define SBA_HD inline
#endif

#define SBA_T 512u            // = SB_BK_T (sb_blocked.hip asserts these four)
#define SBA_OWNP 2u           // = SB_BK_OWNP
#define SBA_OWNB 6u           // = SB_BK_OWNB
#define SBA_OUT 0xFFFFFFF0u   // the offset of a lane with nothing to fetch or store

namespace sba {

// may an array of `bytes` bytes go behind a buffer descriptor?  Every in-range offset is then below SBA_OUT, and below 2^32.
SBA_HD bool fits(uint64_t bytes) { return bytes <= (uint64_t)SBA_OUT; }

// byte offset of element `idx` of an array of `size`-byte elements, for a lane that has one
SBA_HD uint32_t off(bool have, uint32_t idx, uint32_t size) { return have ? size * idx : SBA_OUT; }

// class-relative list index behind entry slot `il` of its class for thread t (sb_blocked.hip SB_ENT_L: a wave's group of two
// slots covers 128 consecutive entries)
SBA_HD uint32_t ent_l(uint32_t t, uint32_t il) { return (il >> 1) * (2u * SBA_T) + t + (t & ~63u) + (il & 1u) * 64u; }

// What a slot names: `have`, and the element index when it does.
struct Slot {
    bool have;
    uint32_t idx;
};
// own particle slot i (r.pos, r.vel, w.pos, w.vel): particle q = t + i T of the tile's n_own, from p0
SBA_HD Slot own_particle(uint32_t t, uint32_t i, uint32_t p0, uint32_t n_own)
{
    const uint32_t q = t + i * SBA_T;
    return Slot{q < n_own, p0 + q};
}
// halo particle slot i (halo_idx): index h = t + i T of the nh_load the launch loads, from h0
SBA_HD Slot halo_index(uint32_t t, uint32_t i, uint32_t h0, uint32_t nh_load)
{
    const uint32_t h = t + i * SBA_T;
    return Slot{h < nh_load, h0 + h};
}
// own entry slot i (last_r, target_r, last_w, target_w, strain, stress): beam j of the tile's n_ownb, from b0
SBA_HD Slot own_beam(uint32_t t, uint32_t i, uint32_t b0, uint32_t n_ownb)
{
    const uint32_t j = ent_l(t, i);
    return Slot{j < n_ownb, b0 + j};
}
// halo entry slot i (ent_state): state index j of the nhe halo entries the launch loads, from s0
SBA_HD Slot halo_state(uint32_t t, uint32_t i, uint32_t s0, uint32_t nhe)
{
    const uint32_t j = ent_l(t, i);
    return Slot{j < nhe, s0 + j};
}
// entry slot i of all SB_BK_MAXB (ent_word, ent_length): own slots count from the tile's first entry e0, halo slots from its
// n_ownb-th; the launch loads ne_load = n_ownb + nhe entries
SBA_HD Slot entry(uint32_t t, uint32_t i, uint32_t e0, uint32_t n_ownb, uint32_t nhe)
{
    if (i < SBA_OWNB) {
        const uint32_t j = ent_l(t, i);
        return Slot{j < n_ownb, e0 + j};
    }
    const uint32_t j = ent_l(t, i - SBA_OWNB);
    return Slot{j < nhe, e0 + n_ownb + j};
}

} // namespace sba
