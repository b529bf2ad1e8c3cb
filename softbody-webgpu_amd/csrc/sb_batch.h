// sb_batch.h -- what the files of the sb_batch_* group share: the device memory of a batch and its host object
// (sb_batch.hip: upload, stepping, state I/O; sb_batch_render.hip: pictures; sb_batch_summary.hip: per-scene statistics, rollouts;
// sb_batch_bodies.hip: connected bodies; sb_batch_contacts.hip: particle and wall contacts; sb_batch_body_summary.hip: statistics per
// body; sb_batch_cut.hip / sb_batch_add.hip / sb_batch_spawn.hip: cuts, welds and spawned particles, the latter two on
// sb_batch_alloc.h, the allocator of their data indices; sb_batch_graph.hip: the beam graph; sb_batch_raycast.hip /
// sb_batch_nearest.hip: range sensors and proximity queries, both on sb_batch_query.h, the plan of a query kernel;
// sb_batch_forces.hip: the next substep's beam and contact forces; sb_batch_pose.hip: the pose of every body against a reference
// shape, on sb_batch_group_sort.h, the sort and ranking it shares with sb_batch_body_summary.hip), and what the
// one-workgroup-per-scene kernels that only read a batch have in common: the scene header each of them opens with (sbb_scene), the
// float <-> ordered-key codec of the reports' extremes and the width of their pinned summation tree (sb_summary_math.h), the
// contact neighbourhood (sb_contact_cells.h, included here: the contact test, the cells' rule, window, selection and buckets); on
// the host the *_kernel_vgprs / *_kernel_scratch_bytes info keys (sbb_kernel_info), the alignment test of the entry points (sbb_misaligned4) and the opening checks of the editing and query calls (sbb_edit_entry).  All of it is
// inline; what only one kernel uses stays in that kernel's file.
#pragma once
#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <string>

#include "../../include/softbody.h"
#include "sb_error.h"
#include "sb_physics.h"
#include "sb_contact_cells.h" // sb_touch, sb_batch_cell_geometry, SbCellWindow, sb_select_ascending, the sb_bucket_* of the LDS cells
#include "sb_summary_math.h" // sbb_finite, sbb_fkey / sbb_unkey, SBB_QNAN, sbb_pow2_at_least: the codec of the report rows

// ---------------------------------------------------------------- device memory of a batch
// Per scene: 32 metadata words (the 112 bytes of the reference's metadata buffer, then SB_BM_B0 / SB_BM_LOADED / SB_BM_P0), a CONSTANT blob
// (what only an upload or an added beam / particle writes) and a STATE blob (what stepping changes), the latter twice: current and reset.  Everything a
// beam or a particle owns is stored at its DATA index, so the state export / import are plain row copies.
#define SB_BM_WORDS 32u
#define SB_BM_P 1u       // metadata.particle_i_c
#define SB_BM_B 6u       // metadata.beam_i_c (live beam slots)
#define SB_BM_CONSTS 12u // 8 physics constants, 8 user input words
#define SB_BM_B0 28u     // beam slots of the reset state (the latest upload, checkpoint or fork); k_batch_reset alone reads it
#define SB_BM_LOADED 29u // 1 once uploaded
#define SB_BM_P0 30u     // particle slots of the reset state; k_batch_reset alone reads it (P0 <= P: only sb_batch_add_particles_device raises P)
#define SB_BATCH_MAT_ROW 6u // length, spring, damp, yield, limit, 1/length

struct SbBatchView {
    uint32_t *meta;     // [n_scenes][SB_BM_WORDS]
    unsigned char *cst; // [n_scenes][cst_bytes]
    unsigned char *st;  // [n_scenes][st_bytes]  current
    unsigned char *rst; // [n_scenes][st_bytes]  reset
    uint32_t cst_bytes, st_bytes; // multiples of 16
    // constant blob: slot -> data index of every particle slot (all max_particles entries of the uploaded mapping, verbatim),
    // per beam DATA index (slot of endpoint A) | (slot of endpoint B) << 16 and the material row, per data index "holds a
    // particle / beam of the upload"
    uint32_t o_pmap, o_bword, o_bmat, o_pex, o_bex;
    // state blob: particle records (6 f32) and beam state {target, last, strain, stress} at their data indices, slot -> data
    // index of every beam slot (verbatim; the delete pass compacts its head in place), pending break flags (one bit per beam
    // SLOT), per beam data index "not removed by a delete pass"
    uint32_t o_part, o_bstate, o_bmap, o_bflags, o_balive;
    uint32_t maxP, maxB, nflagw, n_scenes;
    // contact cells (k_batch_frame<SB_BATCH_CELLS, .>; all zero when the batch walks): G x G cells of side `cell` over
    // [0, bounds]^2, their LDS arrays cell_off bytes into the workgroup's LDS; scenes of at least cell_min_p particles use them;
    // cell_stats[0] / [1]: substeps that ran on the cells / that fell back to the walk because a cell was full
    uint32_t cell_g, cell_off, cell_min_p;
    float cell;
    unsigned long long *cell_stats;
};
// k_batch_frame's COLLIDE parameter
#define SB_BATCH_NO_CONTACTS 0
#define SB_BATCH_WALK 1  // the reference's loop over all slots
#define SB_BATCH_CELLS 2 // the in-LDS cell grid, with the walk as its fallback
// LDS behind cell_off: the buckets of sb_contact_cells.h with their counts twice (one array per substep parity), overflow words u32[2]
static inline uint32_t sb_batch_cell_lds_bytes(uint32_t g) { return (sb_bucket_entry_words(g) + 2u * sb_bucket_count_words(g) + 2u) * 4u; }

SB_DEV uint32_t sbb_uniform(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
SB_DEV float sbb_uniform(float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); }

// ---------------------------------------------------------------- what the report kernels share (one workgroup per scene)
// The header of a scene, workgroup-uniform: `loaded` (0: never uploaded), its particle slots P and live beam slots Bc -- 0 in a
// scene never uploaded, else the metadata's counts, clamped to the capacity (an upload is refused unless they fit; beam slots
// >= Bc are stale: never read) -- and its constant and state blobs.
struct SbbScene {
    uint32_t loaded, P, Bc;
    const unsigned char *cst, *st;
};
SB_DEV SbbScene sbb_scene(const SbBatchView &V, uint32_t scene)
{
    const uint32_t *meta = V.meta + (size_t)scene * SB_BM_WORDS;
    SbbScene s;
    // (metadata words are rewritten between launches by other kernels: read at agent scope, as k_batch_frame does; all three
    // loads are issued before the first is looked at -- the words of a scene never uploaded are zero)
    s.loaded = sbb_uniform(SB_AGENT_LOAD(&meta[SB_BM_LOADED]));
    const uint32_t P = sbb_uniform(SB_AGENT_LOAD(&meta[SB_BM_P])), Bc = sbb_uniform(SB_AGENT_LOAD(&meta[SB_BM_B]));
    s.P = s.loaded ? min(P, V.maxP) : 0u;
    s.Bc = s.loaded ? min(Bc, V.maxB) : 0u;
    s.cst = V.cst + (size_t)scene * V.cst_bytes, s.st = V.st + (size_t)scene * V.st_bytes;
    return s;
}

// ---------------------------------------------------------------- host
struct SbBatchRender; // sb_batch_render.hip
// registers and scratch bytes of one kernel as the runtime reports them (asked for at the first sb_batch_get_info of either)
struct SbbKernelRes {
    int vgprs = -1, scratch = 0;
};

struct sb_batch {
    sb_batch_options opt{};
    std::string err;
    int device = 0;
    hipStream_t stream = nullptr;
    SbBatchView V{};
    SbParams prm{};
    uint32_t subticks = 0, threads = 0, lds_bytes = 0;
    bool mat_lds = false;
    int collide = 0; // SB_BATCH_NO_CONTACTS / _WALK / _CELLS
    uint32_t grid_min_particles = 0; // resolved
    unsigned char *stage = nullptr; // device staging of one upload: meta words, constant blob, state blob
    // sb_batch_fork_device (made at the first fork): per scene the metadata words, the constant blob, the state blob and the reset
    // blob of its source, and the count of entries that named no scene
    unsigned char *fork_stage = nullptr;
    unsigned long long *fork_bad = nullptr;
    size_t fork_stage_bytes = 0;
    uint64_t frames_done = 0, substeps_done = 0;
    int scenes_per_cu = 0, vgprs = 0, scratch = 0;
    SbBatchRender *render = nullptr; // what the renderer keeps between calls (made at the first render)
    SbbKernelRes render_res, summary_res, bodies_res, contacts_res, body_summary_res, cut_res, add_res, graph_res, spawn_res, raycast_res, nearest_res, forces_res, pose_res; // of k_batch_render, k_batch_summary, ...
    bool body_summary_lds_allowed = false; // k_batch_body_summary may be launched with more than 64 KiB of LDS (asked for at the first such launch)
    bool pose_lds_allowed = false;         // likewise k_batch_pose
};

extern thread_local std::string g_batch_create_error; // sb_batch.hip

inline void sb_set_error(sb_batch *b, const char *text) { (b ? b->err : g_batch_create_error) = text; } // (sb_error.h)

static inline sb_status check_launch(sb_batch *b, const char *what)
{
    const hipError_t r = hipGetLastError();
    if (r != hipSuccess) SB_FAIL(b, SB_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(r));
    return SB_OK;
}

// sb_batch_get_info's "<name>_kernel_vgprs" / "<name>_kernel_scratch_bytes" of `kernel`: its registers and scratch bytes as the
// runtime reports them, which `r` keeps; 0 where the runtime does not tell (its error is taken off the record: it must not resurface
// in a later launch check).  false: `key` is neither of the two.
static inline bool sbb_kernel_info(sb_batch *b, const char *name, const void *kernel, SbbKernelRes &r, const char *key, uint64_t *value)
{
    const std::string k(key), n(name);
    const bool want_vgprs = k == n + "_kernel_vgprs";
    if (!want_vgprs && k != n + "_kernel_scratch_bytes") return false;
    if (r.vgprs < 0) {
        hipFuncAttributes fa{};
        if (hipSetDevice(b->device) == hipSuccess && hipFuncGetAttributes(&fa, kernel) == hipSuccess) r.vgprs = fa.numRegs, r.scratch = (int)fa.localSizeBytes;
        else (void)hipGetLastError();
    }
    *value = (uint64_t)std::max(want_vgprs ? r.vgprs : r.scratch, 0);
    return true;
}

// "is one of these device pointers not 4-byte aligned?" (null is aligned: an output that is not asked for)
static inline bool sbb_misaligned4(std::initializer_list<const void *> ptrs)
{
    uintptr_t low = 0;
    for (const void *p : ptrs) low |= (uintptr_t)p;
    return (low & 3u) != 0;
}

// The opening checks of an editing call (sb_batch_cut_device, sb_batch_add_beams_device, sb_batch_add_particles_device; `call`:
// its name in the messages), then the batch's device is selected: a null batch, flag bits outside `known` (known_text: the
// message's list of them), more than k_max `items` ("rows", "shapes") per scene, null items with k > 0, a pointer of `aligned`
// that is not 4-byte aligned (aligned_text: their names).
static inline sb_status sbb_edit_entry(sb_batch *b, const char *call, uint32_t flags, uint32_t known, const char *known_text, uint32_t k,
                                       uint32_t k_max, const char *items, const void *device_items, std::initializer_list<const void *> aligned,
                                       const char *aligned_text)
{
    if (!b) SB_FAIL(b, SB_ERR_INVALID, "%s: null batch", call);
    if (flags & ~known) SB_FAIL(b, SB_ERR_INVALID, "%s: flags 0x%x: only %s known", call, flags, known_text);
    if (k > k_max) SB_FAIL(b, SB_ERR_INVALID, "%s: %u %s per scene, at most %u", call, k, items, k_max);
    if (k && !device_items) SB_FAIL(b, SB_ERR_INVALID, "%s: null %s", call, items);
    if (sbb_misaligned4(aligned)) SB_FAIL(b, SB_ERR_INVALID, "%s: %s must be 4-byte aligned", call, aligned_text);
    SB_HIP(b, hipSetDevice(b->device));
    return SB_OK;
}

static inline uint32_t up16(uint32_t x) { return (x + 15u) & ~15u; }
static inline uint32_t cdivb(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }

void sbb_render_release(sb_batch *b); // sb_batch_render.hip, for sb_batch_destroy
// sb_batch_get_info's keys of one file each (sb_batch_render.hip, sb_batch_summary.hip, ...); false: not one of them
bool sbb_render_info(sb_batch *b, const char *key, uint64_t *value);
bool sbb_summary_info(sb_batch *b, const char *key, uint64_t *value);
bool sbb_bodies_info(sb_batch *b, const char *key, uint64_t *value);
bool sbb_contacts_info(sb_batch *b, const char *key, uint64_t *value);
bool sbb_body_summary_info(sb_batch *b, const char *key, uint64_t *value);
bool sbb_cut_info(sb_batch *b, const char *key, uint64_t *value);
bool sbb_add_info(sb_batch *b, const char *key, uint64_t *value);   // sb_batch_add.hip: add_beams
bool sbb_spawn_info(sb_batch *b, const char *key, uint64_t *value); // sb_batch_spawn.hip: add_particles
bool sbb_graph_info(sb_batch *b, const char *key, uint64_t *value);
bool sbb_raycast_info(sb_batch *b, const char *key, uint64_t *value);
bool sbb_nearest_info(sb_batch *b, const char *key, uint64_t *value);
bool sbb_forces_info(sb_batch *b, const char *key, uint64_t *value); // sb_batch_forces.hip
bool sbb_pose_info(sb_batch *b, const char *key, uint64_t *value);   // sb_batch_pose.hip
