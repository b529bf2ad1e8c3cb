// sb_batch_query.h -- the plan of a batch query kernel (sb_batch_raycast.hip: range sensors; sb_batch_nearest.hip: proximity
// queries): every scene asks its own k <= 256 rows of eight words in ONE launch, one workgroup of 256 per scene.
//   stage    into LDS (sbq_stage): the positions, data indices and (with labels) labels of the particle SLOTS; the live beams as ONE
//            word each -- slot of endpoint A, slot of endpoint B, beam data index: 10 + 10 + 12 bits --; the k rows; k keys of
//            SBQ_NO_KEY.  A beam entry that names nothing (none can be uploaded) is left out: the list is compacted wave by wave, so
//            its order depends on the schedule -- which no output does: minima and counts of integers.
//   walk     the kernel's own two loops.  Thread tid owns row tid % kk (kk: k rounded up to a power of two) and part tid / kk of the
//            256 / kk interleaved parts of both lists (sbq_split), and keeps its smallest key (sb_query_key.h) in registers.  The
//            lanes of a wave that share a part read the same primitive (an LDS broadcast), those of different parts neighbouring
//            words (different banks).  No atomic, no cross-lane step, no barrier inside the loops; part 0 also asks the walls.
//   combine  one LDS atomicMin of the 64-bit key per thread that found something; with k > 128 there is one part and a plain store
//            (sbq_combine; the kernel's barrier follows)
//   answer   one lane per row decodes the key and stores the kernel's own outputs and the hit row (sbq_store_hit: the label is read
//            from the caller's row at the hit's data index, which is inside the row); wave 0 counts the row codes by ballots
//            (sbq_store_counts)
// Nothing of the batch is written; every store goes to the workgroup's own rows.  The key is an integer minimum: the outputs are
// the same bits whatever the schedule.  On the host: the info keys of a query (sbq_info) and the opening of its call (sbq_entry).
#pragma once
#include "sb_batch.h"
#include "sb_query_key.h"

#define SBQ_BLOCK 256u // threads of a workgroup: the most rows of a scene and call
#define SBQ_SLOT_BITS 10u
#define SBQ_SLOT_MASK ((1u << SBQ_SLOT_BITS) - 1u)
#define SBQ_COUNT_WORDS 4u // {valid rows, rows whose answer is a particle, a beam, a wall}
#define SBQ_TAIL_WORDS 4u  // the length of the compacted beam list, padded to 16 bytes

static_assert(SB_BATCH_MAX_PARTICLES <= (1u << SBQ_SLOT_BITS) && SB_BATCH_MAX_BEAMS <= (1u << (32u - 2u * SBQ_SLOT_BITS)),
              "two particle slots and a beam data index share one staged word");
static_assert(SB_BATCH_MAX_PARTICLES <= 0x10000 && SB_BATCH_MAX_BEAMS <= 0x10000, "the index field of a key is 16 bits");
static_assert(SB_BATCH_WALL_LEFT == sbq::WALL_LEFT && SB_BATCH_WALL_RIGHT == sbq::WALL_RIGHT && SB_BATCH_WALL_LOW == sbq::WALL_LOW &&
                  SB_BATCH_WALL_HIGH == sbq::WALL_HIGH, "the wall words");

// LDS of a workgroup: key[256] (8 bytes each, first: aligned), pos[maxP] (2 words each), pidx[maxP], label[maxP], beam[maxB],
// rows[256][8], extra[256][n_extra] (the kernel's own words of a row), the tail
static inline uint32_t sbq_lds_bytes(uint32_t maxP, uint32_t maxB, uint32_t n_extra)
{
    return (2u * SBQ_BLOCK + 4u * maxP + maxB + (SBQ_ROW_WORDS + n_extra) * SBQ_BLOCK + SBQ_TAIL_WORDS) * 4u;
}
struct SbqLds {
    unsigned long long *key; // [256] per row: the smallest key; then its kind
    float2 *pos;             // [maxP] per particle SLOT: position
    uint32_t *pidx;          // [maxP] per SLOT: data index
    int32_t *lab;            // [maxP] per SLOT: the caller's label (-1 without labels)
    uint32_t *beam;          // [maxB] per live beam that names two particles: slot A | slot B << 10 | data index << 20
    uint32_t *row;           // [k][8] the rows
    uint32_t *extra;         // [256][n_extra] per row: the kernel's own words, staged as zeros
    uint32_t *nb;            // [1] beams staged
    uint32_t n_extra;
};
SB_DEV SbqLds sbq_carve(uint32_t *lds, uint32_t maxP, uint32_t maxB, uint32_t n_extra)
{
    SbqLds s;
    s.key = (unsigned long long *)lds;
    s.pos = (float2 *)(lds + 2u * SBQ_BLOCK);
    s.pidx = (uint32_t *)(s.pos + maxP);
    s.lab = (int32_t *)(s.pidx + maxP);
    s.beam = (uint32_t *)(s.lab + maxP);
    s.row = s.beam + maxB;
    s.extra = s.row + SBQ_ROW_WORDS * SBQ_BLOCK;
    s.nb = s.extra + n_extra * SBQ_BLOCK;
    s.n_extra = n_extra;
    return s;
}

// what a query kernel knows of its scene once it is staged (workgroup-uniform)
struct SbqScene {
    uint32_t P, nb;          // particle slots; beams staged
    const uint32_t *g_bword; // per beam DATA index: slot A | slot B << 16
    const float2 *g_part;    // particle records, three float2 each, at their data indices
    const int32_t *lrow;     // the caller's labels of this scene at particle data indices, or null
};
// Stages scene `scene`, its k rows, the keys and the zeros of s.extra.  Two barriers; every thread of the workgroup calls it.  Data
// indices outside the capacity cannot be uploaded; were one met, its particle is nowhere and its beam left out.
SB_DEV SbqScene sbq_stage(const SbBatchView &V, uint32_t scene, const SbqLds &s, const uint32_t *__restrict__ rows, uint32_t k,
                          const int32_t *__restrict__ labels)
{
    const uint32_t tid = threadIdx.x, maxP = V.maxP, maxB = V.maxB;
    const SbbScene hd = sbb_scene(V, scene);
    SbqScene sc;
    sc.P = hd.P;
    const uint32_t P = hd.P, Bc = P ? hd.Bc : 0u; // (a beam needs two particles: an upload is refused unless its endpoints are slots < P)
    const uint32_t *g_pmap = (const uint32_t *)(hd.cst + V.o_pmap), *g_bmap = (const uint32_t *)(hd.st + V.o_bmap);
    sc.g_bword = (const uint32_t *)(hd.cst + V.o_bword);
    sc.g_part = (const float2 *)(hd.st + V.o_part);
    sc.lrow = labels ? labels + (size_t)scene * maxP : nullptr;
    const uint32_t *rrow = rows + (size_t)scene * k * SBQ_ROW_WORDS;

    if (tid == 0u) *s.nb = 0u;
    for (uint32_t p = tid; p < P; p += SBQ_BLOCK) {
        const uint32_t d = g_pmap[p];
        const bool in = d < maxP;
        s.pos[p] = in ? sc.g_part[3u * d] : make_float2(__uint_as_float(SBB_QNAN), __uint_as_float(SBB_QNAN));
        s.pidx[p] = d;
        s.lab[p] = (sc.lrow && in) ? sc.lrow[d] : -1;
    }
    for (uint32_t i = tid; i < k * SBQ_ROW_WORDS; i += SBQ_BLOCK) s.row[i] = rrow[i];
    s.key[tid] = SBQ_NO_KEY;
    for (uint32_t i = 0u; i < s.n_extra; i++) s.extra[s.n_extra * tid + i] = 0u;
    __syncthreads();
    const uint32_t lane = tid & 63u;
    for (uint32_t j0 = 0u; j0 < Bc; j0 += SBQ_BLOCK) { // (uniform trip count: every lane reaches the ballot)
        const uint32_t j = j0 + tid;
        uint32_t word = 0u;
        bool names = false;
        if (j < Bc) {
            const uint32_t d = g_bmap[j];
            if (d < maxB) {
                const uint32_t w = sc.g_bword[d], a = w & 0xffffu, b = w >> 16;
                names = a < P && b < P;
                word = a | (b << SBQ_SLOT_BITS) | (d << (2u * SBQ_SLOT_BITS));
            }
        }
        const unsigned long long m = __ballot(names);
        uint32_t base = 0u;
        if (lane == 0u && m) base = atomicAdd(s.nb, (uint32_t)__popcll(m)); // (at most Bc <= maxB in all: every store below is inside s.beam)
        base = sbb_uniform(base);
        if (names) s.beam[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = word;
    }
    __syncthreads();
    sc.nb = *s.nb;
    return sc;
}
// the endpoints of a staged beam word as slots, and its data index
SB_DEV uint32_t sbq_beam_a(uint32_t word) { return word & SBQ_SLOT_MASK; }
SB_DEV uint32_t sbq_beam_b(uint32_t word) { return (word >> SBQ_SLOT_BITS) & SBQ_SLOT_MASK; }
SB_DEV uint32_t sbq_beam_index(uint32_t word) { return word >> (2u * SBQ_SLOT_BITS); }

// my row and my part of both lists (row >= k: a padding lane, which walks nothing)
struct SbqSplit {
    uint32_t row, part, nparts;
};
SB_DEV SbqSplit sbq_split(uint32_t k)
{
    uint32_t kk = 1u;
    while (kk < k) kk <<= 1; // (uniform; k <= 256)
    return SbqSplit{threadIdx.x & (kk - 1u), threadIdx.x / kk, SBQ_BLOCK / kk};
}
// combines the parts of a row (row < 256 always: a padding lane holds SBQ_NO_KEY); the kernel's barrier follows
SB_DEV void sbq_combine(const SbqLds &s, const SbqSplit &my, uint64_t key)
{
    if (my.nparts > 1u) {
        if (key != SBQ_NO_KEY) atomicMin(&s.key[my.row], (unsigned long long)key);
    } else {
        s.key[my.row] = key;
    }
}

// the slots of the endpoints of the beam a row of `kind` answers with at data index `index` (P and P: it is no beam, or names none)
SB_DEV uint2 sbq_hit_beam(const SbBatchView &V, const SbqScene &sc, int32_t kind, int32_t index)
{
    if (kind != sbq::BEAM || (uint32_t)index >= V.maxB) return make_uint2(sc.P, sc.P);
    const uint32_t w = sc.g_bword[index];
    return make_uint2(w & 0xffffu, w >> 16);
}
// the hit row {kind, index, label} of row `at` of the call; a_slot: sbq_hit_beam's.  The label is the caller's of the particle that
// answers or of the answering beam's endpoint A; -1 for everything else and without labels.
SB_DEV void sbq_store_hit(const SbBatchView &V, const SbqScene &sc, const SbqLds &s, int32_t *__restrict__ out_hit, size_t at, int32_t kind,
                          int32_t index, uint32_t a_slot)
{
    int32_t label = -1;
    if (sc.lrow && (kind == sbq::PARTICLE || kind == sbq::BEAM)) {
        uint32_t p = (uint32_t)index;
        if (kind == sbq::BEAM) p = a_slot < sc.P ? s.pidx[a_slot] : V.maxP;
        if (p < V.maxP) label = sc.lrow[p];
    }
    int32_t *h = out_hit + at * SBQ_HIT_WORDS;
    h[0] = kind, h[1] = index, h[2] = label;
}
// The counts of a scene from each thread's row code (EMPTY on a thread without a row): kinds into s.key -- the thread's own word:
// its row's key was read by this thread alone --, wave 0 counts by ballots.  The last thing every thread of the workgroup does.
SB_DEV void sbq_store_counts(const SbqLds &s, int32_t *__restrict__ counts, uint32_t scene, uint32_t k, int32_t kind)
{
    const uint32_t tid = threadIdx.x;
    if (!counts) return; // (uniform)
    s.key[tid] = (unsigned long long)(uint32_t)kind;
    __syncthreads();
    if (tid >= 64u) return;
    uint32_t n_valid = 0u, n_part = 0u, n_beam = 0u, n_wall = 0u;
    for (uint32_t base = 0u; base < k; base += 64u) { // (uniform trip count)
        const int32_t c = base + tid < k ? (int32_t)(uint32_t)s.key[base + tid] : (int32_t)sbq::EMPTY;
        n_valid += __popcll(__ballot(c >= 0));
        n_part += __popcll(__ballot(c == sbq::PARTICLE));
        n_beam += __popcll(__ballot(c == sbq::BEAM));
        n_wall += __popcll(__ballot(c == sbq::WALL));
    }
    if (tid < SBQ_COUNT_WORDS) counts[(size_t)scene * SBQ_COUNT_WORDS + tid] = (int32_t)(tid == 0u ? n_valid : tid == 1u ? n_part : tid == 2u ? n_beam : n_wall);
}

// ---------------------------------------------------------------- host
// sb_batch_get_info's keys of a query: "<rows>_max", "<rows>_hit_words", "<rows>_count_words", "<name>_lds_bytes" and the two of
// `kernel` (sbb_kernel_info); false: `key` is none of them
static inline bool sbq_info(sb_batch *b, const char *rows, const char *name, uint32_t lds_bytes, const void *kernel, SbbKernelRes &r,
                            const char *key, uint64_t *value)
{
    const std::string k(key), p(rows);
    if (k == p + "_max") *value = SBQ_BLOCK;
    else if (k == p + "_hit_words") *value = SBQ_HIT_WORDS;
    else if (k == p + "_count_words") *value = SBQ_COUNT_WORDS;
    else if (k == std::string(name) + "_lds_bytes") *value = lds_bytes;
    else return sbb_kernel_info(b, name, kernel, r, key, value);
    return true;
}
// The opening checks of a query call: sbb_edit_entry's (no flag is known; `items`: "rays", "points") and "every output is null".
// ptrs: the rows, the labels, then the outputs, whose names outs_text lists.  *launch: there is something to do (k > 0).
static inline sb_status sbq_entry(sb_batch *b, const char *call, uint32_t flags, uint32_t k, const char *items, const char *outs_text,
                                  std::initializer_list<const void *> ptrs, bool *launch)
{
    *launch = false;
    if (!b) SB_FAIL(b, SB_ERR_INVALID, "%s: null batch", call);
    if (std::all_of(ptrs.begin() + 2, ptrs.end(), [](const void *p) { return !p; }))
        SB_FAIL(b, SB_ERR_INVALID, "%s: %s are all null: nothing to write", call, outs_text);
    const std::string aligned = std::string(items) + ", labels, " + outs_text;
    const sb_status st = sbb_edit_entry(b, call, flags, 0u, "no flag is", k, SBQ_BLOCK, items, *ptrs.begin(), ptrs, aligned.c_str());
    *launch = st == SB_OK && k > 0u;
    return st;
}
