// sb_report.h -- what the engine's state calls (sb_state_io.hip), its four whole-scene reports (sb_summary.hip, sb_bodies.hip,
// sb_contacts.hip, sb_body_summary.hip), the cut (sb_cut.hip), the graph (sb_graph.hip), the ray casts (sb_raycast.hip), the proximity queries (sb_nearest.hip) and the forces (sb_forces.hip) share: the owner of their device
// buffers, the preflight of a call, the host mirror of a report, the scene tables of the latest upload, the exclusive scan and
// the wave's run counter.  What only one report uses stays in its file.
#pragma once
#include <vector>

#include "sb_engine.h"
#include "sb_report_tables.h"

// a device block that only ever grows; freed with the engine (sbs_release)
struct SbDevBuf {
    void *p = nullptr;
    size_t cap = 0; // bytes
    sb_status grow(sb_engine *e, size_t bytes); // at least 16 bytes; waits for the stream before a block too small is freed
    void release();
    template <class T> T *as() const { return (T *)p; }
};

// every device buffer the five files keep between calls, by use
enum SbReportBuf {
    SBQ_B_PINV, SBQ_B_TAB, SBQ_B_ISLOT, SBQ_B_MAT,                                 // the shared scene tables (sbq_need)
    SBS_B_SLOT, SBS_B_IMP_ROW, SBS_B_IMP_REST, SBS_B_CKPT,                         // sb_state_io.hip
    SBM_B_BLEAF, SBM_B_PART, SBM_B_STAT, SBM_B_OUT,                                // sb_summary.hip
    SBD_B_PARENT, SBD_B_SIZES, SBD_B_ACC,                                          // sb_bodies.hip
    SBC_B_CELLS, SBC_B_BSUM, SBC_B_SORTED, SBC_B_ABOVE, SBC_B_PLACE, SBC_B_ACC, SBC_B_LABELS, SBC_B_TOUCH, SBC_B_PAIRS, // sb_contacts.hip
    SBY_B_SCRATCH, SBY_B_LABELS, SBY_B_OUT,                                        // sb_body_summary.hip
    SBX_B_ROW, SBX_B_MARK, SBX_B_ACC, SBX_B_SHAPES, SBX_B_HIT,                     // sb_cut.hip (SBX_B_ROW: also sb_graph.hip)
    SBG_B_SCRATCH, SBG_B_ENDS, SBG_B_ROWPTR, SBG_B_NBR, SBG_B_COUNTS,              // sb_graph.hip
    SBW_B_SCRATCH, SBW_B_RAYS, SBW_B_LABELS, SBW_B_T, SBW_B_HIT, SBW_B_COUNTS,      // sb_raycast.hip
    SBV_B_SCRATCH, SBV_B_POINTS, SBV_B_LABELS, SBV_B_D, SBV_B_HIT, SBV_B_POINT, SBV_B_WITHIN, SBV_B_COUNTS, // sb_nearest.hip
    SBF_B_CELLS, SBF_B_BSUM, SBF_B_SORTED, SBF_B_CELL_OF, SBF_B_BEAM, SBF_B_ACC, SBF_B_LABELS, SBF_B_ROWS, SBF_B_BEAM_OUT, SBF_B_TENSION, // sb_forces.hip
    SBQ_NBUF
};

// sb_engine::sio.  Tables of the scene of the latest upload are built at the first call after it that reads them;
// sb_write_buffers drops them all through sbs_invalidate.
struct SbStateIoState {
    SbDevBuf buf[SBQ_NBUF];
    // the shared scene tables, in two parts, the second's fourth plane on its own (sbq_need)
    bool part_valid = false, beam_valid = false, copy_valid = false;
    bool islot_valid = false, mat_valid = false; // sb_forces.hip's two planes: per particle mapping slot the internal particle (SBQ_B_ISLOT); per caller beam slot {spring, damp} (SBQ_B_MAT)
    double islot_ms = 0.0, mat_ms = 0.0;
    uint32_t np = 0, P = 0, nslots = 0; // highest particle data index in use + 1; particles; the caller's beam slots
    std::vector<uint32_t> h_pinv;       // part 1 on the host: part 2's endpoint check reads it
    double part_ms = 0.0, beam_ms = 0.0, copy_ms = 0.0; // host time of each one's last build (copy_ms 0: built with the other planes)
    // sb_read_state_device: per caller slot u {engine slot, data index of its record} (SBS_B_SLOT); the copy is sbr_copy_table's
    bool valid = false;
    // sb_summary.hip: per beam data index < sum_nb {engine slot (0xFFFFFFFF: none), the copy read back for it} (SBM_B_BLEAF)
    bool bleaf_valid = false;
    uint32_t sum_nb = 0, sum_partials = 0; // highest beam data index in use + 1; sb_summary_options.partials as the last call resolved it
    double bleaf_ms = 0.0;
    // sb_write_beams_device: per ENGINE beam slot the data index of its record in the latest upload (0xFFFFFFFF: a beam an upload
    // removed); on the blocked layout also the rest length of every blocked beam, in owner order (the plastic promise's rule)
    bool imp_valid = false;
    double imp_build_ms = 0.0;
    // "<report>_table_build_us": host time of the last build of the tables the report's latest call read (0: no call yet)
    double sum_build_ms = 0.0, bod_build_ms = 0.0, con_build_ms = 0.0, bsm_build_ms = 0.0;
    // sb_checkpoint_device: one block (SBS_B_CKPT) holding a copy of everything a run mutates (sbs_walk_run_state), and the host's words of it
    size_t ckpt_bytes = 0;                    // 0: no checkpoint
    uint32_t ck_cur = 0, ck_bcur = 0, ck_delete_gen = 0;
    uint64_t ck_substeps_done = 0;
    uint64_t checkpoints = 0, restores = 0;   // calls since sb_create
    // sb_cut_device: per caller slot the data index of its beam record (SBX_B_ROW), beside the shared scene tables
    bool cut_valid = false;
    double cut_row_ms = 0.0, cut_build_ms = 0.0;
    uint64_t cuts = 0;                        // calls since sb_create
    uint32_t cut_nd = 0;                      // highest beam data index among the rows + 1 (sb_graph.hip)
    double graph_build_ms = 0.0;              // "graph_table_build_us"
    double ray_build_ms = 0.0;                // "raycast_table_build_us"
    double for_build_ms = 0.0;                // "forces_table_build_us"

    void invalidate() { part_valid = beam_valid = copy_valid = islot_valid = mat_valid = valid = bleaf_valid = imp_valid = cut_valid = false; } // every table of the scene: the one place
};

enum { SBQ_PARTICLES = 1u, SBQ_BEAMS = 2u, SBQ_COPIES = 4u, SBQ_SLOTS = 8u, SBQ_MATERIALS = 16u }; // the parts of the shared scene tables; SBQ_COPIES: part 2's fourth plane; SBQ_SLOTS, SBQ_MATERIALS: sb_forces.hip's planes

inline const char *sbq_options_name(const sb_summary_options *) { return "sb_summary_options"; }
inline const char *sbq_options_name(const sb_bodies_options *) { return "sb_bodies_options"; }
inline const char *sbq_options_name(const sb_contacts_options *) { return "sb_contacts_options"; }
inline const char *sbq_options_name(const sb_body_summary_options *) { return "sb_body_summary_options"; }
inline const char *sbq_options_name(const sb_cut_options *) { return "sb_cut_options"; }
inline const char *sbq_options_name(const sb_graph_options *) { return "sb_graph_options"; }
inline const char *sbq_options_name(const sb_raycast_options *) { return "sb_raycast_options"; }
inline const char *sbq_options_name(const sb_nearest_options *) { return "sb_nearest_options"; }
inline const char *sbq_options_name(const sb_forces_options *) { return "sb_forces_options"; }

sb_status sbq_ready(sb_engine *e, const char *what, const char *why); // loaded, no ranks (`why`: the call's parenthesis); the device; e->sio

// What every report checks before it enqueues, in one order: the options' size, their reserved words, capacities above 2^31
// ("... are not <verb>"), an upload, no ranks; then the device is made current and e->sio exists.  A report's own INVALID checks
// come before the call (they read option fields only where struct_size is exactly the struct's).
template <class O>
sb_status sbq_preflight(sb_engine *e, const char *what, const O *o, const char *verb, const char *why)
{
    if (o && o->struct_size != 0 && o->struct_size != sizeof(O))
        SB_FAIL(e, SB_ERR_INVALID, "%s: %s.struct_size %u != %zu", what, sbq_options_name(o), o->struct_size, sizeof(O));
    if (o && o->struct_size)
        for (uint32_t r : o->reserved)
            if (r) SB_FAIL(e, SB_ERR_INVALID, "%s: reserved option words must be zero", what);
    if (e->opt.max_particles > 0x80000000u || e->opt.max_beams > 0x80000000u)
        SB_FAIL(e, SB_ERR_INVALID, "%s: capacities above 2^31 are not %s", what, verb);
    return sbq_ready(e, what, why);
}

// the mask of beams removed by a delete pass as sb_load_buffers (fetch_dead) sees it: NULL while no pass has removed any
inline const uint32_t *sbq_dead(const sb_engine *e) { return e->B && e->delete_gen ? e->d_dead_gen : nullptr; }

// The host mirror of a report.  One *_enqueue serves both exports of a report: the _device one launches into the caller's device
// memory, the host one into blocks of the engine's, copied to the caller after the launches.  The function names each buffer
// once, through the mirror, and launches into what it gets back; with host == false every operation hands the caller's pointer
// through and finish() does nothing.  A NULL caller pointer is "not wanted" and yields NULL.  out / in / inout record their first
// failure in `st`: check it once, behind the last of them.
struct SbqMirror {
    SbqMirror(sb_engine *e, bool host) : e(e), host(host) {}
    sb_status st = SB_OK;
    // an output of `bytes` bytes in s.buf[buf] (grown to hold it)
    template <class T> T *out(SbReportBuf buf, void *caller, size_t bytes) { return (T *)bind(buf, caller, bytes, bytes, false, true); }
    // an output that lives `offset` bytes into a block the report owns anyway (the counts behind its accumulators)
    template <class T> T *out_at(void *caller, void *block, size_t offset, size_t bytes)
    {
        if (!host || !caller) return (T *)caller;
        back.push_back({caller, (char *)block + offset, bytes});
        return (T *)back.back().dev;
    }
    // an input of `bytes` bytes, uploaded into s.buf[buf] (grown to cap_bytes >= bytes); inout: and copied back with the outputs
    template <class T> const T *in(SbReportBuf buf, const void *caller, size_t bytes, size_t cap_bytes)
    {
        return (const T *)bind(buf, const_cast<void *>(caller), bytes, cap_bytes, true, false);
    }
    template <class T> T *inout(SbReportBuf buf, void *caller, size_t bytes) { return (T *)bind(buf, caller, bytes, bytes, true, true); }
    // behind the launches: the outputs to the caller on e->stream, then the call's one hipStreamSynchronize
    sb_status finish();

private:
    struct Copy { void *caller, *dev; size_t bytes; };
    void *bind(SbReportBuf buf, void *caller, size_t bytes, size_t cap_bytes, bool upload, bool download);
    sb_status stage(SbReportBuf buf, const void *caller, size_t bytes, size_t cap_bytes, bool upload);
    sb_engine *e;
    bool host;
    std::vector<Copy> back;
};

// the most VGPRs (want_vgprs) or scratch bytes over the kernels; false: the runtime refused (the error is taken off the record)
bool sbq_kernel_most(sb_engine *e, const std::vector<const void *> &kernels, bool want_vgprs, uint64_t *value);

// the shared scene tables: builds the parts asked for that the latest upload has not built yet (`what`: the call in messages)
sb_status sbq_need(sb_engine *e, const char *what, uint32_t parts);
// per caller beam slot of the latest upload {engine slot, data index of its record}, both checked against the scene
sb_status sbq_user_slots(sb_engine *e, const char *what, std::vector<uint2> &slots);

// sb_cut.hip: per caller beam slot of the latest upload the data index of its record, on the device (SBX_B_ROW; cut_valid, cut_nd)
sb_status sbx_build_rows(sb_engine *e, const char *what);

// ---- exclusive scan of n 32-bit words into T words (uint32_t / unsigned long long), three launches: a sum per block of SBQ_SCAN
// words into bsum, the block sums scanned in place by ONE workgroup that loops over them with a carry (the sum of all to *total,
// which may be NULL), added back.  `out` may be `in` when T is 32 bits.
#define SBQ_BLOCK 256u
#define SBQ_PER 4u                      // words a thread of a scan block owns
#define SBQ_SCAN (SBQ_BLOCK * SBQ_PER)  // words of a scan block
template <class T>
void sbq_scan(sb_engine *e, const uint32_t *in, uint64_t n, T *bsum, T *out, T *total);
std::vector<const void *> sbq_scan_kernels(bool wide); // the kernels sbq_scan<uint32_t> may launch; wide: and sbq_scan<unsigned long long>'s (the reports' *_kernel_vgprs keys)

// ---- stable LSD radix sort of at most n_max 64-bit keys (the number on the device where n_dev is given) by their bits 32 ..
// 32 + bits - 1, between the buffers a and b; returns the one that holds the result.  It is the body summary's sort
// (sb_body_summary.hip, where its two kernels k_bsum_hist / k_bsum_scatter live), shared with sb_graph.hip.  hist: SBQ_RADIX words per
// block of SBQ_SORT keys; bsum: a word per scan block of hist.
#define SBQ_SORT 1024u
#define SBQ_RADIX 256u
unsigned long long *sbq_sort(sb_engine *e, unsigned long long *a, unsigned long long *b, uint32_t n_max, const uint32_t *n_dev, uint32_t bits,
                             uint32_t *hist, uint32_t *bsum);
std::vector<const void *> sbq_sort_kernels();

// The length of the run for the first lane of each maximal run of equal keys in the wave, 0 for every other lane and for a run
// that is not valid.  Every lane of the wave calls it.
SB_DEV uint32_t sbq_run_length(uint32_t key, bool valid)
{
    const uint32_t lane = __lane_id();
    const uint32_t left = __shfl_up(key, 1);
    const bool head = lane == 0u || left != key;
    const unsigned long long heads = __ballot(head);
    if (!(head && valid)) return 0u;
    const unsigned long long rest = lane == 63u ? 0ull : heads >> (lane + 1u);
    return rest ? (uint32_t)__ffsll(rest) : 64u - lane; // up to the next head, or to the end of the wave
}

// one atomicAdd per wave on a count word: how many of its lanes say `mine`.  Every lane of the wave calls it.
SB_DEV void sbw_count(unsigned long long *acc, uint32_t word, bool mine)
{
    const unsigned long long m = __ballot(mine);
    if (m && __lane_id() == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(&acc[word], (unsigned long long)__popcll(m));
}

// ---- the uniform grid of the whole scene (sb_raycast.hip; csrc/sb_ray_walk.h states the cells' rule and what is recorded where),
// shared by the ray casts and the proximity queries: the grid of a call, and the counting sort of particles, short beams and the
// leftover list into it -- memsets, k_ray_bin, sbq_scan, k_ray_bin -- enqueued on the engine's stream.
namespace srw {
struct Grid;
struct Rec;
}
struct SbwSortPlan {
    uint64_t nbin, nb_scan, items; // words of the bins (G * G cells, the leftover list, one behind), blocks of their scan, records at most
};
srw::Grid sbw_grid(const sb_engine *e, uint32_t cells_per_side); // cells_per_side 0: the default rule
SbwSortPlan sbw_sort_plan(const sb_engine *e, uint32_t G);
// acc: the eight count words (k_ray_bin takes words 5 and 6) and whatever lies behind them, acc_bytes in all, cleared; d_cells [nbin]:
// afterwards per bin the END of its records; bsum [nb_scan]; sorted [items]; a_of: per beam data index < cut_nd its endpoint A, or NULL;
// *total: the number of records
sb_status sbw_sort(sb_engine *e, const srw::Grid &g, unsigned long long *acc, size_t acc_bytes, uint32_t *d_cells, uint32_t *bsum, srw::Rec *sorted,
                   uint32_t *a_of, uint32_t *total);
std::vector<const void *> sbw_sort_kernels(); // what sbw_sort launches (the *_kernel_vgprs keys)
