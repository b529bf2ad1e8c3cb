// sb_report_tables.h -- the scene tables of the latest upload that the engine's whole-scene reports read (sb_report.hip uploads
// what these return).  Part 1: per particle DATA index below np (the highest in use + 1) the internal particle
// holding it (h_pidx inverted; SBQ_NONE where none lives).  Part 2: per caller beam slot of the latest upload the four planes
// {data index of A, data index of B, engine slot, the copy read back for it}; the fourth only once a report asks for it.  Two more planes for sb_forces.hip, each on first use: per particle mapping SLOT the
// internal particle holding it (h_pslot inverted), and per caller beam slot its {spring, damp} as uploaded.  Everything a kernel will index with is checked here,
// once: a defect names the first kind of fault found.  Header-only and HIP-free: tests/report_tables_check.cpp runs it under
// AddressSanitizer / ThreadSanitizer.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "sb_tiling.h" // SbHostBeam, sbt::parallel_ranges

#define SBQ_NONE 0xFFFFFFFFu

namespace sbq {

enum Defect { OK = 0, BAD_PARTICLE_INDEX, BAD_BEAM_SLOT, BAD_ENDPOINT, BAD_COPY, BAD_PARTICLE_SLOT };

inline const char *defect_text(Defect d)
{
    switch (d) {
    case BAD_PARTICLE_INDEX: return "particle data index outside the scene";
    case BAD_BEAM_SLOT: return "beam slot outside the scene";
    case BAD_ENDPOINT: return "beam endpoint outside the scene";
    case BAD_COPY: return "beam copy outside the scene";
    case BAD_PARTICLE_SLOT: return "particle mapping slot outside the scene";
    default: return "";
    }
}

// the first (smallest) defect any thread met
inline void note(std::atomic<uint32_t> &bad, Defect d)
{
    uint32_t was = bad.load(std::memory_order_relaxed);
    while ((was == OK || (uint32_t)d < was) && !bad.compare_exchange_weak(was, (uint32_t)d, std::memory_order_relaxed)) {}
}

// pinv[d] = the internal particle i with pidx[i] == d, d < *np = the highest data index in use + 1 (one entry of SBQ_NONE for an
// empty scene: nothing is uploaded from an empty vector).  pidx holds every data index once (the upload's own check).  Two serial
// passes: a round of threads costs more than it saves at a million particles.
inline Defect invert_particles(const uint32_t *pidx, size_t P, uint32_t max_particles, std::vector<uint32_t> &pinv, uint32_t *np)
{
    uint32_t top = 0; // (32-bit words and raw pointers: both loops stay as cheap as they can be)
    for (size_t i = 0; i < P; i++) top = std::max(top, pidx[i]);
    if (P && top >= max_particles) return BAD_PARTICLE_INDEX;
    *np = P ? top + 1u : 0u;
    pinv.assign(std::max<uint32_t>(*np, 1), SBQ_NONE);
    uint32_t *const to = pinv.data();
    for (size_t i = 0; i < P; i++) to[pidx[i]] = (uint32_t)i;
    return OK;
}

// The planes of [4][n = max(nslots, 1)] that `planes` names, packed in that order into tab: ENDS = {data index of A, data index of B,
// engine slot}, COPY = {the copy read back}.  user_slot: caller slot -> engine slot, strictly increasing (NULL: the identity);
// beams / copy_of_slot: per engine slot < B.  Checked: the slot is < B; with ENDS, both endpoints name a data index < np at which a
// particle lives; with COPY, the copy is < nbeam.
enum { ENDS = 1u, COPY = 2u };
inline Defect beam_planes(unsigned planes, const uint32_t *user_slot, size_t nslots, const SbHostBeam *beams, const uint32_t *copy_of_slot,
                          uint32_t B, uint32_t nbeam, const std::vector<uint32_t> &pinv, uint32_t np, std::vector<uint32_t> &tab)
{
    const size_t n = std::max<size_t>(nslots, 1);
    const bool ends = planes & ENDS, copy = planes & COPY;
    tab.assign(((ends ? 3 : 0) + (copy ? 1 : 0)) * n, 0u);
    uint32_t *const t = tab.data(), *const tc = t + (ends ? 3 : 0) * n;
    std::atomic<uint32_t> bad{OK};
    sbt::parallel_ranges(nslots, 1 << 16, [&](size_t u0, size_t u1) {
        for (size_t u = u0; u < u1; u++) {
            const uint32_t slot = user_slot ? user_slot[u] : (uint32_t)u;
            if (slot >= B) {
                note(bad, BAD_BEAM_SLOT);
                continue;
            }
            const SbHostBeam &h = beams[slot];
            if (ends && (h.da >= np || h.db >= np || pinv[h.da] == SBQ_NONE || pinv[h.db] == SBQ_NONE)) {
                note(bad, BAD_ENDPOINT);
                continue;
            }
            if (copy && copy_of_slot[slot] >= nbeam) {
                note(bad, BAD_COPY);
                continue;
            }
            if (ends) t[u] = h.da, t[n + u] = h.db, t[2 * n + u] = slot;
            if (copy) tc[u] = copy_of_slot[slot];
        }
    });
    return (Defect)bad.load();
}

// islot[s] = the internal particle i with pslot[i] == s, s < P (the sibling of invert_particles' table: the particle mapping slots of
// an upload are 0 .. P - 1, each once; one entry of SBQ_NONE for an empty scene).  A slot outside 0 .. P - 1, or one that two
// particles claim, is a defect: sb_forces_device fetches the partners of a particle through this table.
inline Defect invert_slots(const uint32_t *pslot, size_t P, std::vector<uint32_t> &islot)
{
    islot.assign(std::max<size_t>(P, 1), SBQ_NONE);
    uint32_t *const to = islot.data();
    for (size_t i = 0; i < P; i++) {
        const uint32_t s = pslot[i];
        if (s >= P || to[s] != SBQ_NONE) return BAD_PARTICLE_SLOT;
        to[s] = (uint32_t)i;
    }
    return OK;
}

// mat[2 u], mat[2 u + 1] = {spring, damp} of caller beam slot u < nslots as uploaded (SbHostBeam::f[3], f[4]: materials never change
// between uploads), n = max(nslots, 1) pairs; user_slot as in beam_planes.  Checked: the slot is < B.
inline Defect beam_materials(const uint32_t *user_slot, size_t nslots, const SbHostBeam *beams, uint32_t B, std::vector<float> &mat)
{
    mat.assign(2 * std::max<size_t>(nslots, 1), 0.0f);
    float *const m = mat.data();
    std::atomic<uint32_t> bad{OK};
    sbt::parallel_ranges(nslots, 1 << 16, [&](size_t u0, size_t u1) {
        for (size_t u = u0; u < u1; u++) {
            const uint32_t slot = user_slot ? user_slot[u] : (uint32_t)u;
            if (slot >= B) {
                note(bad, BAD_BEAM_SLOT);
                continue;
            }
            m[2 * u] = beams[slot].f[3], m[2 * u + 1] = beams[slot].f[4];
        }
    });
    return (Defect)bad.load();
}

} // namespace sbq
