// sb_scene_codec.h -- the ONE place that knows the reference's scene buffers (engineMapping.ts:103-370): metadata header, mapping
// entries (u16 in v1, u32 in v2), beam records (v1: a | b << 16, nine floats at +4; v2: a, b, nine floats at +8), what sizes
// the four buffers must have, and what makes a scene valid.  Keyed by layout and capacity, not by who asks: sb_engine (sb_api.hip),
// sb_batch (sb_batch.hip) and the partitioner (sb_partition.cpp) all read and write records through it, so they cannot disagree.
// It formats no messages: errors come back as values and every caller words its own.  Header-only and HIP-free:
// tests/scene_codec_check.cpp runs it under AddressSanitizer / ThreadSanitizer.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/softbody.h"
#include "sb_tiling.h" // sbt::parallel_ranges, sbt::uvec

namespace sbc {

constexpr uint32_t NONE = 0xFFFFFFFFu;

inline uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

// ---------------------------------------------------------------- layout facts
inline uint32_t map_item_bytes(uint32_t layout) { return layout == SB_LAYOUT_V1 ? 2u : 4u; }
inline uint32_t beam_stride(uint32_t layout) { return layout == SB_LAYOUT_V1 ? SB_BEAM_STRIDE_V1 : SB_BEAM_STRIDE_V2; }
inline uint32_t beam_floats_offset(uint32_t layout) { return layout == SB_LAYOUT_V1 ? 4u : 8u; }
inline size_t mapping_bytes(uint32_t layout, uint32_t maxP, uint32_t maxB) { return ((size_t)maxP + maxB) * map_item_bytes(layout); }

// ---------------------------------------------------------------- mapping entries (particle slots first, beam slots from maxP on)
inline uint32_t map_get(uint32_t layout, const uint8_t *m, size_t id)
{
    if (layout == SB_LAYOUT_V1) {
        uint16_t v;
        memcpy(&v, m + 2 * id, 2);
        return v;
    }
    return rd32(m + 4 * id);
}
inline void map_set(uint32_t layout, uint8_t *m, size_t id, uint32_t val)
{
    if (layout == SB_LAYOUT_V1) {
        const uint16_t v = (uint16_t)val;
        memcpy(m + 2 * id, &v, 2);
    } else {
        memcpy(m + 4 * id, &val, 4);
    }
}

// ---------------------------------------------------------------- one beam record (engineMapping.ts:183-186, compute.wgsl:99-100)
// a, b: the endpoints as particle DATA indices; f9: length, target_length, last_length, spring, damp, yield_strain,
// strain_break_limit, strain, stress -- as the 36 bytes they occupy (a caller's buffer need not be aligned: copy them out)
inline void decode_beam(uint32_t layout, const uint8_t *rec, uint32_t &a, uint32_t &b, const uint8_t *&f9)
{
    if (layout == SB_LAYOUT_V1) {
        const uint32_t pair = rd32(rec);
        a = pair & 0xffffu;
        b = pair >> 16;
    } else {
        a = rd32(rec);
        b = rd32(rec + 4);
    }
    f9 = rec + beam_floats_offset(layout);
}
inline void encode_beam(uint32_t layout, uint8_t *rec, uint32_t a, uint32_t b, const void *f9)
{
    if (layout == SB_LAYOUT_V1) {
        const uint32_t pair = (a & 0xffffu) | (b << 16);
        memcpy(rec, &pair, 4);
    } else {
        memcpy(rec, &a, 4);
        memcpy(rec + 4, &b, 4);
    }
    memcpy(rec + beam_floats_offset(layout), f9, 9 * sizeof(float));
}

// ---------------------------------------------------------------- buffer sizes
enum Buffer : uint32_t { BUF_OK = 0, BUF_NULL, BUF_METADATA, BUF_MAPPING, BUF_PARTICLES, BUF_BEAMS };
struct SizeError { uint32_t buffer = BUF_OK; size_t have = 0, need = 0; }; // BUF_NULL: a buffer that has to be there is not
inline const char *buffer_name(uint32_t buffer)
{
    static const char *const names[] = {"", "null", "metadata", "mapping", "particle", "beam"};
    return names[buffer <= BUF_BEAMS ? buffer : 0];
}
// need_all: an upload (every buffer must be there; beams may be null at capacity 0).  Otherwise a read-back: null = not wanted.
inline SizeError check_sizes(uint32_t layout, uint32_t maxP, uint32_t maxB, bool need_all, const void *metadata, size_t metadata_bytes,
                             const void *mapping, size_t mapping_bytes_, const void *particles, size_t particles_bytes, const void *beams,
                             size_t beams_bytes)
{
    if (need_all && (!metadata || !mapping || !particles || (!beams && maxB))) return {BUF_NULL, 0, 0};
    const struct { uint32_t buffer; const void *p; size_t have, need; } all[4] = {
        {BUF_METADATA, metadata, metadata_bytes, SB_METADATA_BYTES},
        {BUF_MAPPING, mapping, mapping_bytes_, mapping_bytes(layout, maxP, maxB)},
        {BUF_PARTICLES, particles, particles_bytes, (size_t)maxP * SB_PARTICLE_STRIDE},
        {BUF_BEAMS, beams, beams_bytes, (size_t)maxB * beam_stride(layout)},
    };
    for (const auto &b : all)
        if (b.p && b.have < b.need) return {b.buffer, b.have, b.need};
    return {};
}

// ---------------------------------------------------------------- metadata header (compute.wgsl:29-54)
struct Header {
    uint32_t P, B, maxP, maxB; // active particle / beam slots, capacities
    explicit Header(const uint8_t *md) : P(rd32(md + 4)), B(rd32(md + 24)), maxP(rd32(md + 40)), maxB(rd32(md + 44)) {}
    bool capacity_is(uint32_t p, uint32_t b) const { return maxP == p && maxB == b; }
    bool counts_fit(uint32_t p, uint32_t b) const { return P <= p && B <= b; }
};

// ---------------------------------------------------------------- scene validation
// The rule: particle slots map to distinct data indices below capacity, beam slots likewise, and both endpoints of every beam
// are particles that some slot maps to.
enum ErrorKind : uint32_t { SCENE_OK = 0, PARTICLE_RANGE, PARTICLE_TWICE, BEAM_RANGE, BEAM_TWICE, ENDPOINT };
struct SceneError {
    uint32_t kind = SCENE_OK;
    uint32_t slot = NONE; // the offending slot (of two slots that share a data index: the later one)
    uint32_t idx = 0;     // the data index it maps to
    uint32_t a = 0, b = 0; // ENDPOINT: the record's endpoints (data indices); PARTICLE_TWICE: a = the slot that mapped idx first
};
// the offence a single walk in slot order would meet first
inline bool before(const SceneError &x, const SceneError &y)
{
    return x.kind && (!y.kind || x.slot < y.slot || (x.slot == y.slot && x.kind < y.kind));
}

struct Scene {
    uint32_t layout, maxP, maxB, P, B; // counts within capacity (Header::counts_fit)
    const uint8_t *mapping, *beams;    // beams may be null while B == 0
};

// particle slots: data_of_slot[P], slot_of_data[maxP] (NONE: no slot maps to it)
inline SceneError map_particles(const Scene &sc, std::vector<uint32_t> &data_of_slot, std::vector<uint32_t> &slot_of_data)
{
    data_of_slot.resize(sc.P);
    slot_of_data.assign(sc.maxP, NONE);
    for (uint32_t s = 0; s < sc.P; s++) {
        const uint32_t idx = map_get(sc.layout, sc.mapping, s);
        if (idx >= sc.maxP) return {PARTICLE_RANGE, s, idx, 0, 0};
        if (slot_of_data[idx] != NONE) return {PARTICLE_TWICE, s, idx, slot_of_data[idx], 0};
        slot_of_data[idx] = s;
        data_of_slot[s] = idx;
    }
    return {};
}

// what on_beam(const BeamSlot &) is told about every valid beam slot, once, from the thread that walks its range
struct BeamSlot {
    uint32_t slot, idx; // beam slot, beam data index
    uint32_t a, b;      // endpoints as particle SLOTS
    uint32_t da, db;    // endpoints as particle data indices (what the record holds)
    const uint8_t *f9;  // the record's nine floats (decode_beam)
};

// Beam slots [s0, s1), callable side by side from several threads over disjoint ranges.  `claimed` [maxB], NONE at the start and
// shared by all of them: the lowest slot seen so far per beam data index -- of two slots that share one, the LATER is reported
// whichever thread comes second, so the answer does not depend on the schedule.  Returns the range's lowest offence; a range stops
// at the first offence of its own (what lies behind it cannot be the scene's first).
template <typename OnBeam>
inline SceneError check_beam_range(const Scene &sc, const uint32_t *slot_of_data, uint32_t *claimed, size_t s0, size_t s1, OnBeam on_beam)
{
    SceneError mine;
    const uint32_t stride = beam_stride(sc.layout);
    for (size_t i = s0; i < s1; i++) {
        const uint32_t s = (uint32_t)i, idx = map_get(sc.layout, sc.mapping, (size_t)sc.maxP + s);
        if (idx >= sc.maxB) {
            const SceneError here{BEAM_RANGE, s, idx, 0, 0};
            return before(here, mine) ? here : mine;
        }
        uint32_t prev = __atomic_load_n(&claimed[idx], __ATOMIC_RELAXED);
        while (s < prev && !__atomic_compare_exchange_n(&claimed[idx], &prev, s, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
        if (prev != NONE) {
            const SceneError here{BEAM_TWICE, std::max(prev, s), idx, 0, 0};
            if (before(here, mine)) mine = here;
            if (here.slot == s) return mine;
        }
        BeamSlot r{s, idx, 0, 0, 0, 0, nullptr};
        decode_beam(sc.layout, sc.beams + (size_t)idx * stride, r.da, r.db, r.f9);
        if (r.da >= sc.maxP || r.db >= sc.maxP || slot_of_data[r.da] == NONE || slot_of_data[r.db] == NONE) {
            const SceneError here{ENDPOINT, s, idx, r.da, r.db};
            return before(here, mine) ? here : mine;
        }
        r.a = slot_of_data[r.da];
        r.b = slot_of_data[r.db];
        on_beam(r);
    }
    return mine;
}

// every beam slot, in ONE walk on a few host threads (sbt::parallel_ranges); the offence at the lowest slot is the one reported
template <typename OnBeam>
inline SceneError check_beams(const Scene &sc, const std::vector<uint32_t> &slot_of_data, OnBeam on_beam)
{
    sbt::uvec<uint32_t> claimed(sc.maxB);
    sbt::parallel_ranges(sc.maxB, (size_t)1 << 18, [&](size_t i0, size_t i1) { std::fill(claimed.begin() + i0, claimed.begin() + i1, NONE); });
    std::mutex m;
    std::vector<SceneError> per_range;
    sbt::parallel_ranges(sc.B, (size_t)1 << 15, [&](size_t s0, size_t s1) {
        const SceneError mine = check_beam_range(sc, slot_of_data.data(), claimed.data(), s0, s1, on_beam);
        if (!mine.kind) return;
        std::lock_guard<std::mutex> lock(m);
        per_range.push_back(mine);
    });
    SceneError first;
    for (const SceneError &e : per_range)
        if (before(e, first)) first = e;
    return first;
}

template <typename OnBeam>
inline SceneError validate_scene(const Scene &sc, std::vector<uint32_t> &data_of_slot, std::vector<uint32_t> &slot_of_data, OnBeam on_beam)
{
    const SceneError e = map_particles(sc, data_of_slot, slot_of_data);
    return e.kind ? e : check_beams(sc, slot_of_data, on_beam);
}

} // namespace sbc
