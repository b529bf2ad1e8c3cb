/*
 * softbody.h -- C ABI of the MI355X-native softbody physics step.
 *
 * Drop-in boundary for ONE path of spsquared/softbody-webgpu: the per-substep
 * physics step (`compute_update` / `compute_delete`, src/shaders/compute.wgsl:90-246)
 * as driven by src/engineWorker.ts.  The reference has no FFI: its boundary is the
 * set of WebGPU calls engineWorker.ts makes on seven storage buffers, in the byte
 * layouts src/engineMapping.ts defines.  Each entry point below replaces one of
 * those call groups (cited per function) and moves raw bytes in those layouts.
 *
 * Conventions
 *   - plain C types only; every function returns an sb_status (0 = ok);
 *     sb_last_error() gives the message for the last failure on that engine
 *     (engine == NULL: the last sb_create failure of the calling thread).
 *   - COPY semantics: no host pointer is retained after a call returns (the JS
 *     ArrayBuffers are owned and later mutated by BufferMapper,
 *     engineMapping.ts:364-367).
 *   - one call at a time per engine, like the reference's AsyncLock
 *     (src/lock.ts:4-19; engineWorker.ts:553,584,632).  When do calls return?
 *       SB_COLLIDE_OFF / SB_COLLIDE_ALLPAIRS, and SB_PATH_ATOMIC with any collision mode:
 *         sb_step / sb_frame / sb_delete_pass only ENQUEUE work on the engine's HIP stream;
 *         sb_sync, sb_load_buffers, sb_step_timed and sb_render wait for it.
 *       SB_COLLIDE_GRID on the tiled path (the default of sb_default_options): sb_step and
 *         sb_frame MAY WAIT for the stream, like every call of the reference does
 *         (engineWorker.ts:632-633,686-688: `await queue.onSubmittedWorkDone()` on both
 *         sides of a frame).  The spatial hash keeps itself valid on the device; what
 *         the host owes it is one look when a call's substeps have been issued (did a
 *         substep move somebody farther than predicted?  -- then the launches behind it
 *         returned at once and are issued again behind a fresh hash), and the stretches
 *         that run several substeps per launch (nothing within reach of anything) are
 *         sized from a look at the device as well.  So a call returns when its LAST
 *         substep has been issued and everything before the last look has run: for a
 *         1 M-particle scene a 64-substep frame holds the calling thread for about
 *         2.4 ms of its 2.4 ms (a Node host should call from a worker thread, as the
 *         reference itself does: engine.ts:138).  sb_delete_pass, sb_write_user_input
 *         and the sb_halo_* / sb_peer_* calls still only enqueue.
 *       Any collision mode and path: sb_render waits for the stream, sb_render_device only enqueues.
 *       sb_read_state_device and sb_write_particles_device only enqueue (the first export after an upload builds its tables
 *         and waits for the stream once, as the first render does; with SB_COLLIDE_GRID the import's reset of the spatial
 *         hash copies its start state from host memory, which the runtime may do behind the work in flight).
 *       The sb_batch_* group (many small scenes, below): everything only enqueues on the batch's own stream except
 *         sb_batch_write_scene, sb_batch_load_scene and sb_batch_sync, which wait for it.
 *         sb_batch_render_device only enqueues; sb_batch_render_scene waits for the stream.
 *       A wait POLLS the stream for as long as the work in flight should take (busily for
 *         the first 8 ms, then every ~50 us between short sleeps; 0.2 s at most) before it
 *         parks the thread: being woken costs 0.2 - 0.5 ms on some hosts, more than many
 *         of these waits.  SB_WAIT_SPIN_US=0 in the environment parks always.
 *   - there is no CPU fallback: without a usable HIP device sb_create fails.
 */
#ifndef SOFTBODY_H
#define SOFTBODY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SB_ABI_VERSION 1

typedef struct sb_engine sb_engine;

typedef enum sb_status {
    SB_OK = 0,
    SB_ERR_INVALID = 1,     /* bad argument / buffer too small / inconsistent scene */
    SB_ERR_HIP = 2,         /* a HIP runtime call failed (message carries hipGetErrorString) */
    SB_ERR_NO_DEVICE = 3,   /* no usable gfx950 device (engineWorker.ts:86,93,98 throw TypeError) */
    SB_ERR_OOM = 4,
    SB_ERR_STATE = 5,       /* call order (e.g. step before write_buffers) */
    SB_ERR_UNSUPPORTED = 6
} sb_status;

/* host buffer layouts (src/engineMapping.ts) */
#define SB_LAYOUT_V1 1 /* reference: u16 mapping, beam = packed u16 pair + 9 f32, stride 40 */
#define SB_LAYOUT_V2 2 /* wide: u32 mapping, beam = u32 a, u32 b + 9 f32, stride 44 */

/* particle-particle collision broad phase (compute.wgsl:142-170) */
#define SB_COLLIDE_OFF 0      /* skip the collision loop (BASELINE config 2) */
#define SB_COLLIDE_ALLPAIRS 1 /* the reference's O(P^2) scan, LDS-tiled */
#define SB_COLLIDE_GRID 2     /* spatial hash + neighbour lists; same pair set and summation order => same bits
                               * as SB_COLLIDE_ALLPAIRS.  The default (sb_default_options). */

/* device schedule of one substep */
#define SB_PATH_AUTO 0
#define SB_PATH_ATOMIC 1 /* beam kernel with global i32 atomics + particle kernel */
#define SB_PATH_TILED 2  /* fused LDS-tiled substep: forces never leave the CU */

#define SB_METADATA_BYTES 112
#define SB_PARTICLE_STRIDE 24
#define SB_BEAM_STRIDE_V1 40
#define SB_BEAM_STRIDE_V2 44
#define SB_USER_INPUT_BYTES 32
#define SB_USER_INPUT_OFFSET 80

typedef struct sb_options {
    uint32_t struct_size;    /* = sizeof(sb_options) */
    float bounds_size;       /* engineWorker.ts:39 (fixed 1000 there; an option here) */
    float particle_radius;   /* engineWorker.ts:40,89 */
    uint32_t subticks;       /* engineWorker.ts:41,90: rounded UP to even; time_step = 1/subticks (:331) */
    uint32_t max_particles;  /* capacity; BufferMapper.maxParticles (engineMapping.ts:362) */
    uint32_t max_beams;      /* capacity; BufferMapper.maxBeams (engineMapping.ts:363) */
    uint32_t layout;         /* SB_LAYOUT_* */
    uint32_t collision_mode; /* SB_COLLIDE_* */
    uint32_t path;           /* SB_PATH_* */
    uint32_t tile_particles; /* SB_PATH_TILED: target particles per tile (0 = the engine picks: fewest rounds of resident tiles).
                              * An UPPER BOUND where several substeps run per launch (collisions off, or nothing within reach): a tile of
                              * that kernel owns at most 1024 particles and 3072 beams, larger targets are lowered to fit */
    int32_t device_ordinal;  /* HIP device */
    float grid_skin;         /* SB_COLLIDE_GRID: cells are 2r + 2*skin wide and the hash is rebuilt only when
                              * some particle may have moved more than `skin` (relative to the scene's common
                              * drift) since the last build.  0 = default: adaptive, starting at 0.4 r; a hash that
                              * is worn out within 3 substeps is followed by one with the smallest doubled skin (up
                              * to 1.6 r) that promises two substeps, one that lasted 64 by one half as wide; > 0 =
                              * that skin, fixed; negative = rebuild every substep */
    uint32_t block_substeps; /* SB_PATH_TILED: substeps one launch advances out of LDS and registers (temporal
                              * blocking over beam-hop rings; same bits as single substeps).  With SB_COLLIDE_OFF
                              * always; with SB_COLLIDE_GRID for the stretches of a run in which every neighbour
                              * list of the spatial hash is empty (the collision loop is then a no-op; the engine
                              * tracks what the particles move and redoes, substep by substep, a launch that used
                              * up the hash's skin).
                              * 0 = default: a plan 7 substeps deep, each call cut into the cheapest balanced
                              * launches (long calls 6 per launch, 20 substeps as 7 + 7 + 6); N > 1 = every call in
                              * the fewest launches of at most N (at most 8); 1 = one launch per substep.  Lowered
                              * automatically to the deepest plan whose regions fit the kernel's registers and LDS */
    uint32_t reserved[3];
} sb_options;

/* Fill with the reference defaults: bounds 1000, radius 10, subticks 64, 65536/65536, v1,
 * spatial-hash collisions (the bits of the reference's all-pairs scan), auto path, device 0. */
void sb_default_options(sb_options *opts);

/* Replaces the WGPUSoftbodyEngineWorker constructor's device/buffer/pipeline creation
 * (engineWorker.ts:83-176, 312-343). */
sb_status sb_create(const sb_options *opts, sb_engine **out);

/* engineWorker.ts:711-717 destroy(). */
sb_status sb_destroy(sb_engine *e);

/* Replaces writeBuffers() (engineWorker.ts:580-597): uploads metadata, mapping, particle data
 * (-> buffer A) and beam data; zeroes the force accumulators, the delete mask and buffer B.
 * Buffers are the BufferMapper ArrayBuffers (engineMapping.ts:342-345) at FULL capacity:
 * metadata 112 B, mapping (max_particles+max_beams) entries, particles max_particles*24 B,
 * beams max_beams*stride B; the *_bytes arguments are checked against that.
 * An upload with the topology of the scene already on the device (same counts and mapping, every beam between the same
 * two particles with the same rest length and material; no ghost zones configured) keeps the engine's plan and only moves
 * state -- about a tenth of the time of an upload that plans (sb_get_info "uploads_kept" counts them); the results are
 * those of a fresh engine either way.  So does an upload that only REMOVED beams from that scene (at most an eighth of them; the
 * beams that are left in their old order under any valid mapping, which is what BufferMapper.writeState produces after
 * removeBeam calls or after a run whose delete passes removed beams, engineMapping.ts:452-459,500-518): the removed beams die on
 * the device like beams a delete pass removed, counts / records / mapping read back exactly as from a fresh engine
 * ("uploads_edited" counts those).  An upload that ADDS a beam plans again. */
sb_status sb_write_buffers(sb_engine *e, const void *metadata, size_t metadata_bytes,
                           const void *mapping, size_t mapping_bytes,
                           const void *particles, size_t particles_bytes,
                           const void *beams, size_t beams_bytes);

/* Replaces Metadata.writeUserInput (engineMapping.ts:323-325, engineWorker.ts:636-642):
 * the 32 bytes at metadata offset 80 (user_strength, mouse_active, mouse_pos, mouse_vel,
 * applied_force). */
sb_status sb_write_user_input(sb_engine *e, const void *bytes32);

/* Replaces the PHYSICS_CONSTANTS round trip (engineWorker.ts:497-507): the 8 floats at
 * metadata offset 48 (gravity.xy, border_elasticity, border_friction, elasticity, friction,
 * drag_coeff, drag_exp), without re-uploading the scene. */
sb_status sb_set_physics_constants(sb_engine *e, const float constants8[8]);
sb_status sb_get_physics_constants(sb_engine *e, float constants8[8]);

/* Replaces the compute pass of frame() (engineWorker.ts:646-665): `subticks` x compute_update
 * with alternating read/write particle buffers, then one compute_delete. */
sb_status sb_frame(sb_engine *e);

/* n x compute_update only (benchmark granularity: one "step" = one substep).  Any n; the
 * engine tracks which particle buffer is current. */
sb_status sb_step(sb_engine *e, uint32_t n_substeps);

/* one compute_delete (compute.wgsl:205-246, canonical semantics: stable compaction). */
sb_status sb_delete_pass(sb_engine *e);

/* device.queue.onSubmittedWorkDone() (engineWorker.ts:633,687). */
sb_status sb_sync(sb_engine *e);

/* sb_step bracketed by HIP events on the engine's stream; *ms = device time of the n substeps. */
sb_status sb_step_timed(sb_engine *e, uint32_t n_substeps, float *ms);

/* Time marks that do not stop the host: sb_mark records HIP event number `slot` (0 .. SB_MAX_MARKS-1) at the current end of
 * the engine's stream and returns at once; sb_mark_elapsed waits for mark b and gives the device time from mark a to mark
 * b.  For loops that interleave sb_step with other stream work (the ghost refresh of the multi-GPU path: the bench times
 * the substep launches and the exchanges of every rank this way without a host synchronisation per exchange). */
#define SB_MAX_MARKS 4096
sb_status sb_mark(sb_engine *e, uint32_t slot);
sb_status sb_mark_elapsed(sb_engine *e, uint32_t a, uint32_t b, float *ms);

/* Replaces loadBuffers() (engineWorker.ts:548-579): metadata, mapping, particles (current
 * buffer) and beams back into host ArrayBuffers of full capacity.  Only records reachable
 * through the mapping are written; other bytes of the caller's buffers are left as they are.
 * Any pointer may be NULL to skip that buffer. */
sb_status sb_load_buffers(sb_engine *e, void *metadata, size_t metadata_bytes,
                          void *mapping, size_t mapping_bytes,
                          void *particles, size_t particles_bytes,
                          void *beams, size_t beams_bytes);

/* counts as the device sees them (metadata.particle_i_c / beam_i_c after deletes). */
sb_status sb_get_counts(sb_engine *e, uint32_t *particles, uint32_t *beams);

/* introspection for benches/tests: key = "path", "tiles", "beam_copies", "halo_particles",
 * "device_bytes", "substeps_done", "kernels_per_substep", "substep_hbm_bytes" (the HBM bytes one substep
 * launch has to move with the data layout the engine holds: the launched kernel's own compulsory traffic),
 * "grid_cells", "grid_builds", "grid_wide", "grid_skin_x1000", "material_mode", "materials", "local_index_bits",
 * "blocked_word_format" (how the blocked kernel holds the plan's entry words: 0 wide, as in memory; 1 narrow, repacked per launch),
 * "render_table_build_us" (host time of sb_render's last draw-table build: the first render after an upload),
 * "render_wide_particles" / "render_wide_beams" (how many particles / beams the latest sb_render or sb_render_device drew with a
 * wave each rather than in their own thread: a clipped box of more than 64 pixels, more than 32 clipped points; 0 before the
 * first render.  Both wait for the stream and copy two words to the host: for tests, never inside a timed region),
 * "halo_guard" (1 while a halo guard is set, sb_halo_guard),
 * "summary_partials" (sb_summary: the partials the last call used), "summary_table_build_us" (host time of the last build of the tables
 * its latest call read: the scene tables the reports share and its own; 0 before its first call), "summary_kernel_vgprs" / "summary_kernel_scratch_bytes" (the most registers / scratch
 * bytes per lane over every kernel a summary may launch, as the runtime reports them; scratch must be 0),
 * "bodies_table_build_us" (sb_bodies: host time of the last build of the shared scene tables its latest call read; 0 before its first call), "bodies_kernel_vgprs" /
 * "bodies_kernel_scratch_bytes" (the same two figures over every kernel sb_bodies may launch; scratch must be 0),
 * "contacts_table_build_us" (sb_contacts: host time of the last build of the shared scene table its latest call read; 0 before its first call),
 * "contacts_cells_per_side" (the cells per side its counting sort uses for the scene as it is now; 1: the all-pairs test),
 * "contacts_kernel_vgprs" / "contacts_kernel_scratch_bytes" (the same two figures over every kernel sb_contacts may launch),
 * "body_summary_table_build_us" (sb_body_summary: host time of the last build of the shared scene tables its latest call read; 0 before its first call),
 * "body_summary_scratch_bytes" (device bytes its calls hold so far: scratch, labels, the two scene tables it reads, sb_body_summary's result),
 * "body_summary_kernel_vgprs" /
 * "body_summary_kernel_scratch_bytes" (the same two figures over every kernel sb_body_summary may launch; scratch must be 0),
 * "acc_dirty_tiles" / "plastic_tiles" (tiles whose zero-acceleration / never-yielded promise flag in the CURRENT state
 * buffer is nonzero; 0 on engines without tiles, "plastic_tiles" 0 without a blocked plan.  Both wait for the stream and
 * copy one word per tile to the host: for tests, never inside a timed region),
 * "state_half" (0 / 1: the particle buffer, and with it the row of acceleration flags, that is current; every substep launch
 * flips it), "beam_state_half" (0 / 1: the current half of the blocked layout's target / last-length / plastic double buffers;
 * 0 without a blocked plan).  Both read host words only: tests assert the half an import, checkpoint or restore ran on. */
sb_status sb_get_info(sb_engine *e, const char *key, uint64_t *value);

/* ---- multi-GPU halo exchange; one engine per rank/GPU, each holding its
 * slab of the scene PLUS a ghost zone k beam-hops deep copied from its neighbours.  Ghost
 * particles and ghost beams are stepped like any others (redundantly; the arithmetic is
 * deterministic, so the copies agree bit for bit while their inputs are valid); every k substeps
 * the owners overwrite them: p,v,a (6 floats) per ghost particle, target_length,last_length
 * (2 floats) per ghost beam.  Lists are DATA indices into this engine's particle / beam buffers,
 * in the order the peer packs them.  The exchange itself (RCCL send/recv on the packed device
 * buffers) is the caller's; see softbody-webgpu_amd/halo.py. */
sb_status sb_halo_configure(sb_engine *e, const uint32_t *ghost_particles, uint32_t n_ghost_particles,
                            const uint32_t *send_particles, uint32_t n_send_particles,
                            const uint32_t *ghost_beams, uint32_t n_ghost_beams,
                            const uint32_t *send_beams, uint32_t n_send_beams);
/* Optional: where each list entry lives inside the packed buffers, as FLOAT offsets (6 floats per
 * particle entry, 2 per beam entry).  Default (or NULL): all particles back to back, then all beams.
 * A caller with several neighbours uses this to make each neighbour's share one contiguous segment
 * (one send and one receive per neighbour).  Call after sb_halo_configure. */
sb_status sb_halo_set_layout(sb_engine *e, const uint32_t *send_particle_off, const uint32_t *send_beam_off,
                             const uint32_t *ghost_particle_off, const uint32_t *ghost_beam_off);
/* current state of the send lists -> DEVICE buffer of (6*n_send_particles + 2*n_send_beams) floats
 * (particles first), enqueued on the engine's stream. */
sb_status sb_halo_pack(sb_engine *e, void *device_dst);
/* DEVICE buffer of (6*n_ghost_particles + 2*n_ghost_beams) floats -> current state of the ghost
 * lists, enqueued on the engine's stream. */
sb_status sb_halo_unpack(sb_engine *e, const void *device_src);
/* Beams that BREAK in a multi-GPU run.  A flagged beam keeps acting until the delete pass at the end of its frame
 * (compute.wgsl:205-246, engineWorker.ts:663-664), so only that pass has to agree between ranks, and a beam must
 * disappear from every rank that holds a copy in the same pass.  The owner decides: on an engine with a halo
 * sb_delete_pass drops the flags the GHOST copies raised themselves (their inputs may have been invalid) and removes
 * the rest; from then on the owner's record of a removed beam travels as "dead" in every pack (a NaN payload in
 * last_length); unpack flags the local copies of such beams, and sb_halo_delete_ghosts removes them.  A frame on
 * every rank is therefore:  substeps with a refresh every `depth` of them  ->  sb_delete_pass  ->  one more refresh
 * (pack / exchange / unpack, or sb_peer_exchange)  ->  sb_halo_delete_ghosts.   halo.py Exchanger.frame() and
 * host/halo.js PeerExchanger.frame() do exactly that. */
sb_status sb_halo_delete_ghosts(sb_engine *e);
/* ---- direct neighbour exchange over peer mappings (xGMI stores into the neighbour's mailbox) ----
 * The alternative to moving the packed buffers with a collective library: every exchange is three
 * launches on the engine's own stream (pack straight into the neighbours' mailboxes, signal + wait,
 * unpack), no host synchronisation.  A mailbox is fine-grained device memory: 64 u32 sequence flags
 * (256 B), then two receive buffers (alternating by exchange parity) of the packed receive layout,
 * each rounded up to 256 B.  Order of calls: sb_halo_configure [+ sb_halo_set_layout] ->
 * sb_peer_mailbox on every rank -> trade the 64-byte handles -> sb_peer_map for each neighbour in
 * another process (a neighbour engine in the same process passes its local pointer directly) ->
 * sb_peer_connect -> sb_peer_exchange whenever the ghost zone must be refreshed.  Every rank must
 * call sb_peer_exchange the same number of times.  A neighbour that does not show up within
 * `timeout_ms` makes the wait give up (no hung wave): the next sb_sync reports SB_ERR_HIP. */
#define SB_MAX_PEERS 8
sb_status sb_peer_mailbox(sb_engine *e, void **local_mailbox, void *ipc_handle_64_bytes, uint64_t *mailbox_bytes);
sb_status sb_peer_map(sb_engine *e, const void *ipc_handle_64_bytes, void **mapped_mailbox);
/* per neighbour j: its mailbox, the float count of ITS packed receive layout, my send segment
 * [send_begin, send_begin+send_len) (floats, in my packed send layout), where that segment starts in
 * its receive layout (floats), and which flag slot of its mailbox is mine (= my position in its
 * neighbour order).  My own flag slot for neighbour j is j. */
sb_status sb_peer_connect(sb_engine *e, uint32_t n_peers, void *const *mailboxes, const uint32_t *peer_recv_floats,
                          const uint32_t *send_begin, const uint32_t *send_len, const uint32_t *dst_begin,
                          const uint32_t *their_slot, uint32_t timeout_ms);
sb_status sb_peer_exchange(sb_engine *e);

/* ---- generic x-slab partition of ANY scene into per-rank scenes with ghost zones (host only, no GPU needed) ----
 * The reference has no counterpart (one browser tab, one GPU); this is what lets a scene built by BufferMapper
 * (engineMapping.ts:432-527) or loaded from a snapshot (:407-430) run on several GPUs.  Input: the four host
 * buffers of sb_write_buffers.  owner(particle) = equal-population slab of its x coordinate; ghosts of a rank =
 * everything within `depth` beam hops of its own particles and (contact_reach > 0) of every particle whose x lies
 * within contact_reach of the x range of its own particles (so that contacts across slab faces are computed on
 * both sides: choose at least depth * max(2r + the distance a particle moves in one substep, the longest beam)).  Every rank's scene keeps
 * the relative order of slots and of data indices, so the collision loop's slot order and its index tie-break
 * (compute.wgsl:144,153) are those of the whole scene.  owner(beam) = owner of its endpoint A.  Exchange every
 * `depth` substeps (sb_halo_* / sb_peer_*): both sides list the traded records in ascending GLOBAL data index.
 * Errors are reported through sb_last_error(NULL).  Limits: ghost zones are redundant computation, valid while
 * information travels at most one hop per substep -- contacts between particles of slabs that are not neighbours
 * in x are missed, and break flags do not cross ranks.  Ownership never migrates: sb_halo_guard says when to partition again. */
typedef struct sb_partition sb_partition;
sb_status sb_partition_create(uint32_t layout, uint32_t max_particles, uint32_t max_beams, const void *metadata, const void *mapping,
                              const void *particles, const void *beams, uint32_t world, uint32_t depth, float contact_reach,
                              sb_partition **out);
sb_status sb_partition_destroy(sb_partition *p);
/* counts = { local particles, local beams, owned particles, owned beams, peers, depth, global particles, global beams } */
sb_status sb_partition_rank_counts(const sb_partition *p, uint32_t rank, uint32_t counts[8]);
/* the layout the partition was created with (SB_LAYOUT_V1 / SB_LAYOUT_V2): it fixes the record sizes of what
 * sb_partition_rank_scene writes -- mapping indices of 2 or 4 bytes, beam records of SB_BEAM_STRIDE_V1 or _V2 bytes */
sb_status sb_partition_layout(const sb_partition *p, uint32_t *layout);
/* the rank's scene in the partition's layout, into caller buffers of the given capacities (>= the local counts) */
sb_status sb_partition_rank_scene(const sb_partition *p, uint32_t rank, uint32_t max_particles, uint32_t max_beams, void *metadata,
                                  void *mapping, void *particles, void *beams);
/* per LOCAL data index: the global data index and whether this rank owns it (any pointer may be NULL) */
sb_status sb_partition_rank_ids(const sb_partition *p, uint32_t rank, uint32_t *particle_global, uint8_t *particle_owned,
                                uint32_t *beam_global, uint8_t *beam_owned);
/* peer j (ascending rank): its rank and the lengths { ghost particles, sent particles, ghost beams, sent beams } ... */
sb_status sb_partition_peer_counts(const sb_partition *p, uint32_t rank, uint32_t j, uint32_t *peer_rank, uint32_t counts[4]);
/* ... and the lists themselves, LOCAL data indices in the order sb_halo_configure expects (any pointer may be NULL) */
sb_status sb_partition_peer_lists(const sb_partition *p, uint32_t rank, uint32_t j, uint32_t *ghost_particles, uint32_t *send_particles,
                                  uint32_t *ghost_beams, uint32_t *send_beams);

/* halo guard data of one rank (world <= 64, else SB_ERR_UNSUPPORTED; see sb_halo_guard), as fixed at partition time:
 * lo[world], hi[world] = the x-extent of every rank's own particles (+inf / -inf for a rank that owns none);
 * geometry = { R: the contact reach (0 for world 1), H: the hop length SB_GUARD_HOP_HEADROOM * max(2 * particle_radius,
 * longest live beam) }; held[local particles] = per LOCAL data index, bit t set when rank t holds the particle (own or ghost).
 * Any output pointer may be NULL. */
#define SB_GUARD_HOP_HEADROOM 1.5f
sb_status sb_partition_rank_guard(const sb_partition *p, uint32_t rank, float particle_radius, float *lo, float *hi, float geometry[2],
                                  uint64_t *held);

/* ---- halo guard: the device notices when a partition has gone stale ----
 * Ghost zones are fixed when the scene is partitioned and ownership never migrates, so once particles move far enough a rank
 * misses contacts it should compute and its owned state silently stops matching the single engine.  An engine with a guard
 * runs one more kernel at the end of every ghost refresh (behind the unpack of sb_halo_unpack and of sb_peer_exchange), on the
 * engine's stream, that checks the rule below on the refreshed state -- the ghost endpoint of a beam that crosses ranks is then
 * its owner's copy; sb_halo_guard_status reads the verdict.  NOTE: a rank without neighbours must still call sb_halo_unpack
 * (NULL buffer, empty lists) or sb_peer_exchange at each of its refreshes: those calls are where the check runs.  The guard only reads state.
 *   Fixed at partition time (sb_partition_rank_guard): lo_t, hi_t per rank t, R, H; the caller adds depth D (substeps between
 *   refreshes, at most) and s, the motion allowance per substep (0 = default H / (16 D)).  C = D * (H + s), the chain reach.
 *   At every refresh, on the refreshed state (float32 arithmetic in exactly this order; a check FAILS when its comparison is false,
 *   so NaN fails (A), (C), (D)):
 *     (A) own particle:  lo_r - (R - 3C) <= x <= hi_r + (R - 3C)
 *     (B) own particle, every rank t != r that does not hold it:  NOT (lo_t - (R - C) <= x <= hi_t + (R - C))
 *     (C) own beam (endpoint A owned) that no delete pass has removed:  sqrt(dx*dx + dy*dy) <= H - (2D) * s
 *     (D) own particle:  |x - x at the previous refresh| <= n * s, n = substeps since then
 *   With SB_COLLIDE_OFF, or world 1, only (C) and (D) are checked.  If every check passes at every refresh and no particle moves more than s
 *   in x within one substep, every owned state equals the single engine's bit for bit.  Blind spot: (D) sees the
 *   displacement between refreshes only, so a particle that leaves and returns within one refresh window goes unnoticed.
 * Call order: sb_halo_configure [+ sb_halo_set_layout] -> sb_halo_guard -> refreshes -> sb_halo_guard_status.  Errors:
 * SB_ERR_STATE before sb_halo_configure; SB_ERR_UNSUPPORTED for world > 64; SB_ERR_INVALID for a bad rank or index, depth 0,
 * H or s not finite, s > H / 2, H - 2Ds <= 0, or (collisions on) R < 3C, with a message.  A NULL desc turns the guard off; so
 * do a new upload and a new sb_halo_configure.  sb_get_info "halo_guard" = 1 while a guard is set. */
#define SB_GUARD_SLAB 1u   /* (A) an own particle left its slab */
#define SB_GUARD_BAND 2u   /* (B) a particle entered the band of a rank that does not hold it */
#define SB_GUARD_BEAM 4u   /* (C) an own beam is longer than H allows */
#define SB_GUARD_MOTION 8u /* (D) an own particle moved more than the allowance */
typedef struct sb_halo_guard_desc {
    uint32_t struct_size;          /* = sizeof(sb_halo_guard_desc) */
    uint32_t rank, world, depth;
    float contact_reach;           /* R */
    float hop;                     /* H */
    float motion;                  /* s per substep; 0 = H / (16 depth) */
    uint32_t n_own_particles;
    const uint32_t *own_particles; /* local particle data indices */
    const uint64_t *held;          /* per own particle (same order): bit t = rank t holds it */
    uint32_t n_own_beams;
    const uint32_t *own_beams;     /* local beam data indices */
    const float *lo, *hi;          /* [world] */
    uint32_t reserved[4];
} sb_halo_guard_desc;
typedef struct sb_halo_guard_report {
    uint32_t kinds;         /* SB_GUARD_* bits of every failed check since sb_halo_guard */
    uint32_t violations;    /* (refresh, item) pairs that failed at least one check */
    uint32_t refreshes;     /* refreshes checked */
    uint32_t first_refresh; /* index of the first refresh that failed (0 = the first refresh after sb_halo_guard); ~0 = none */
    uint32_t first_is_beam; /* the first failed item at that refresh (particles before beams, lowest data index first): */
    uint32_t first_index;   /* its LOCAL data index */
    float motion;           /* the s in use */
    uint32_t reserved;
} sb_halo_guard_report;
sb_status sb_halo_guard(sb_engine *e, const sb_halo_guard_desc *desc);
/* waits for the engine's stream, then reads the verdict */
sb_status sb_halo_guard_status(sb_engine *e, sb_halo_guard_report *report);

/* ---- pictures of the state (the reference's render pass, engineWorker.ts:666-683) ----
 * The picture is that of the headless renderer host/render.js, renderPPM(mapper, {resolution, boundsSize, particleRadius})
 * with `mapper` holding what sb_load_buffers would return at this point of the stream, BYTE FOR BYTE: the PPM body, RGB8,
 * resolution^2 * 3 bytes, rows top to bottom, no "P6" header.  One disc per particle slot (inner (0,89,128) within 0.8 r,
 * white ring up to r), then one line per live beam slot coloured by its stress / strain, later slots over earlier ones.
 * The engine evaluates render.js's double arithmetic step for step and resolves "last writer wins" by an integer max over
 * per-pixel keys, so the bytes do not depend on the schedule.  Where render.js does not terminate (a particle with an
 * infinite coordinate, a beam with a non-finite endpoint coordinate, or pixel coordinates of 2^53 and beyond) the engine
 * draws nothing for that primitive; a particle with a NaN coordinate draws nothing in both.
 * Zero fields mean: resolution 512 (render.js's default); bounds_size and particle_radius those of sb_options.
 * Errors: SB_ERR_STATE before an upload; SB_ERR_INVALID for a resolution above 16384 or a buffer smaller than
 * resolution^2 * 3 bytes; SB_ERR_UNSUPPORTED on an engine with ghost zones configured (ranks are not composited).
 * A render only reads the state: it changes nothing a later step, frame or read-back computes.
 * sb_render WAITS for the stream and copies into host memory; sb_render_device only ENQUEUES on the engine's stream
 * and writes into device memory (a torch tensor, say), which must stay valid until that work has run. */
#define SB_RENDER_MAX_RESOLUTION 16384
typedef struct sb_render_options {
    uint32_t struct_size;    /* = sizeof(sb_render_options); 0 or a NULL pointer = all defaults */
    uint32_t resolution;     /* picture is resolution x resolution pixels; 0 = 512 */
    double bounds_size;      /* world units across the picture; 0 = sb_options.bounds_size */
    double particle_radius;  /* disc radius in world units; 0 = sb_options.particle_radius */
    uint32_t reserved[4];
} sb_render_options;
sb_status sb_render(sb_engine *e, const sb_render_options *opts, void *rgb, size_t rgb_bytes);
sb_status sb_render_device(sb_engine *e, const sb_render_options *opts, void *device_rgb);

/* ---- the state in device memory (no host round trip) ----
 * These calls only ENQUEUE on the engine's stream; the device buffers must stay valid until that work has run.  The first export
 * after an upload builds its beam tables and waits for the stream once, as the first render does; later calls only enqueue.
 * Errors: SB_ERR_STATE before an upload; SB_ERR_UNSUPPORTED on an engine with ghost zones or peers configured (ranks are not
 * handled here); SB_ERR_INVALID for a NULL source to sb_write_particles_device, or a particle buffer that is not 8-byte / a beam
 * buffer that is not 16-byte aligned.
 *
 * sb_read_state_device -- any pointer may be NULL:
 *   particles:  max_particles * 24 B, the particle record (6 f32: p.xy, v.xy, a.xy) at each particle's DATA index: exactly the
 *               bytes sb_load_buffers would write into its particle buffer at this point of the stream.
 *   beams:      max_beams * 16 B, 4 f32 { target_length, last_length, strain, stress } at each beam's data index (the data indices
 *               of the latest upload's mapping; a beam a delete pass removed keeps its last state, as in sb_load_buffers).
 *   beam_alive: max_beams bytes, 1 = live, 0 = removed by a delete pass (or by a plan-keeping upload), per data index.
 *   Data indices that hold no particle / beam of the latest upload are NOT written.  Reading only reads: the state, the spatial
 *   hash, the per-tile flags and the schedule stay as they were, and every later result is the one without the call. */
sb_status sb_read_state_device(sb_engine *e, void *device_particles, void *device_beams, void *device_beam_alive);

/* sb_write_particles_device -- overwrites p, v, a of every particle from a device buffer in the particle layout above (only the
 * records at the data indices of the scene's particles are read).  Beams, counts, pending break flags, the mapping and the substep
 * count are untouched.  Every later result is the one the engine would compute had its particle state been these bytes all along.
 * The spatial hash starts again (as after an upload that keeps the plan) and the hybrid schedule looks at the scene afresh.  An
 * import that moves particles far from where the last planning upload saw them stays correct but may run slower until the next
 * planning upload: the hash keeps the frame fitted at that upload (particles outside are clamped into its edge cells), and the
 * tiles stay those bisected from the upload's positions. */
sb_status sb_write_particles_device(sb_engine *e, const void *device_particles);

/* sb_write_beams_device -- overwrites target_length and / or last_length of every beam of the latest upload from a device buffer
 * in sb_read_state_device's beam layout (max_beams * 16 B, { target_length, last_length, strain, stress } at beam DATA indices; only
 * the rows of the latest upload's beams are read, through the latest mapping -- also after an upload that cut beams).  fields:
 * SB_BEAM_TARGET_LENGTH and / or SB_BEAM_LAST_LENGTH (zero or any other bit: SB_ERR_INVALID); strain and stress are never
 * imported.  Every copy the engine keeps of a beam is written.  A removed beam's row is written but inert: a later export shows the
 * imported floats, nothing else changes.  Counts, the mapping, pending break flags, the substep count and the particles are
 * untouched; the spatial hash and the hybrid schedule stay as they are (beams do not move particles).  Every later result is the one
 * the engine would compute had those floats been these bytes all along; values move bit for bit (NaN payloads, -0.0).  Only
 * enqueues; the first call after an upload builds a table and waits for the stream once.  Errors as above; SB_ERR_INVALID also for
 * a NULL source or a buffer that is not 16-byte aligned (checked, like `fields`, before anything touches a device). */
#define SB_BEAM_TARGET_LENGTH 1u
#define SB_BEAM_LAST_LENGTH   2u
sb_status sb_write_beams_device(sb_engine *e, const void *device_beams, uint32_t fields);

/* sb_checkpoint_device / sb_restore_device -- going back without the host.  A checkpoint is a copy of everything a run mutates
 * (particles, beam state, per-tile promise flags, pending break flags, the beams delete passes removed, the substep count), held in
 * device memory of the engine's: one per engine, a later one replaces it; every sb_write_buffers (plan-keeping or not),
 * sb_halo_configure and sb_destroy drop it.  After sb_restore_device, sb_load_buffers, sb_get_counts, sb_read_state_device, every
 * report (summary, bodies, contacts, body_summary, render), sb_get_info "substeps_done" and every later step / frame / delete pass
 * give the bits the engine gave -- or would have given -- at and after the checkpoint, on every path and collision mode: also for a
 * checkpoint taken mid-frame with break flags pending, and across delete passes that removed beams since.  Physics constants and
 * user input are NOT part of it: they stay as they are now.  The spatial hash starts again and the hybrid schedule looks at the
 * scene afresh, as after sb_write_particles_device.  Several restores from one checkpoint are allowed; sb_restore_device without a
 * checkpoint is SB_ERR_STATE.  The first checkpoint after an upload allocates (SB_ERR_OOM: the engine is unchanged and there is no
 * checkpoint) and may wait for the stream once; later checkpoints, and every restore, only enqueue.  sb_get_info:
 * "checkpoint_bytes" (device bytes the checkpoint holds; 0: none), "checkpoints" and "restores" (calls since sb_create). */
sb_status sb_checkpoint_device(sb_engine *e);
sb_status sb_restore_device(sb_engine *e);

/* ---- cutting beams on the device: knife strokes and eraser discs ----
 * "Cut what this stroke crosses", "erase what lies under this disc" -- without reading the scene back, removing beams on the host
 * and uploading again.  A cut raises, for every beam it hits, the break flag the substep would have raised had the beam broken:
 * from then on the beam is in exactly the state of one that broke in the last substep.  It still acts until the next delete pass
 * (sb_frame's own, or sb_delete_pass), which removes it; until then it shows in sb_get_info "beams_flagged", in the pending counts
 * of the summaries, and in a checkpoint.
 *
 * A SHAPE is 8 words, sb_cut_shape: { kind, x0, y0, x1, y1, 0, 0, 0 }; kind is an integer word, the coordinates are floats.
 *   SB_CUT_NONE     ignored
 *   SB_CUT_SEGMENT  a knife from P = (x0, y0) to Q = (x1, y1)
 *   SB_CUT_DISC     an eraser with centre C = (x0, y0) and radius r = x1; y1 must be 0
 * THE PREDICATE (csrc/sb_cut_math.h), float32, one rounding per operator, in the order written; A, B are the positions of the
 * beam's endpoints in the particle state at the call's place in the stream.
 *   Segment: orient(u, v, w) = (v.x - u.x) * (w.y - u.y) - (v.y - u.y) * (w.x - u.x); d1 = orient(P, Q, A), d2 = orient(P, Q, B),
 *     d3 = orient(A, B, P), d4 = orient(A, B, Q); inbox(u, v, w): min(u.x, v.x) <= w.x <= max(u.x, v.x), and the same in y.  A hit iff
 *       ((d1 > 0 && d2 < 0) || (d1 < 0 && d2 > 0)) && ((d3 > 0 && d4 < 0) || (d3 < 0 && d4 > 0)), or
 *       d1 == 0 && inbox(P, Q, A), or d2 == 0 && inbox(P, Q, B), or d3 == 0 && inbox(A, B, P), or d4 == 0 && inbox(A, B, Q).
 *   Disc: d = B - A, w = C - A, L2 = d.x * d.x + d.y * d.y, t = w.x * d.x + w.y * d.y, r2 = r * r.  Never a hit unless r >= 0;
 *     if !(t > 0): a hit iff w.x * w.x + w.y * w.y <= r2; else if t >= L2: with u = C - B, iff u.x * u.x + u.y * u.y <= r2;
 *     else with c = d.x * w.y - d.y * w.x, iff c * c <= r2 * L2.
 *   No division, no square root.  Every comparison with a NaN is false, so a NaN in a beam or in a shape hits nothing.  An
 *   infinity follows the operators like any other number (Inf - Inf and 0 * Inf are NaN, the rest compares): an infinite radius
 *   over a finite beam is a hit.
 * A beam is HIT when any shape of the call hits it.  Only LIVE beams of the latest upload are tested: the caller's beam slots that
 * neither a delete pass nor a plan-keeping upload has removed (a beam whose flag is already pending is live).
 *
 * Outputs, each may be NULL:
 *   hit    [max_beams] bytes: 1 / 0 per beam DATA index of the latest upload's beams (0 for a removed beam); indices that hold no
 *          beam of the latest upload are NOT written, as in sb_read_state_device.
 *   counts [SB_CUT_COUNT_WORDS] int64, exact: tested (live beams tested), hit, flagged (hit beams whose flag this call raised;
 *          0 in a dry run), already_flagged (hit beams whose flag was pending before the call).
 * flags: SB_CUT_DRY_RUN reports and raises no flag.  Every copy the engine's layout keeps of a hit beam gets its bit.  Particles,
 * beam floats, the spatial hash and the hybrid schedule are untouched, exactly as sb_write_beams_device leaves them.
 * sb_cut_device only ENQUEUES on the engine's stream: shapes and outputs are device memory, which must stay valid until that
 * work has run.  The first call after an upload builds its tables on the host and waits for the stream once; no host copy of
 * positions is read.  sb_cut takes host memory, WAITS and copies back.
 * Errors, all before anything touches a device: SB_ERR_INVALID for a NULL handle, a struct_size that is neither 0 nor the
 * struct's, a nonzero reserved word, unknown flag bits, n_shapes > SB_CUT_MAX_SHAPES, NULL shapes with n_shapes > 0, shapes that
 * are not 4-byte or counts that are not 8-byte aligned, a capacity above 2^31; sb_cut also for a kind outside { 0, 1, 2 } and a disc
 * with y1 != 0 (sb_cut_device cannot see the shapes: such a shape hits nothing).  SB_ERR_STATE before an upload;
 * SB_ERR_UNSUPPORTED on an engine with ghost zones or peers configured.  n_shapes == 0 is a valid call: nothing is hit, `tested`
 * is still reported.  sb_get_info: "cuts" (calls since sb_create), "cut_table_build_us", "cut_kernel_vgprs". */
#define SB_CUT_NONE 0u
#define SB_CUT_SEGMENT 1u
#define SB_CUT_DISC 2u
#define SB_CUT_MAX_SHAPES 64u
#define SB_CUT_COUNT_WORDS 4u
#define SB_CUT_DRY_RUN 1u
typedef struct sb_cut_shape {
    uint32_t kind;           /* SB_CUT_NONE / SB_CUT_SEGMENT / SB_CUT_DISC */
    float x0, y0, x1, y1;    /* segment: P, Q; disc: centre, radius, 0 */
    uint32_t reserved[3];    /* zero */
} sb_cut_shape;
typedef struct sb_cut_options {
    uint32_t struct_size;    /* = sizeof(sb_cut_options); 0 or a NULL pointer = all defaults */
    uint32_t flags;          /* SB_CUT_DRY_RUN */
    uint32_t reserved[6];    /* zero */
} sb_cut_options;
sb_status sb_cut_device(sb_engine *e, const sb_cut_options *opts, const void *device_shapes /* [n_shapes] sb_cut_shape */,
                        uint32_t n_shapes, void *device_hit_u8 /* [max_beams] or NULL */,
                        void *device_counts_i64 /* [SB_CUT_COUNT_WORDS] int64 or NULL */);
sb_status sb_cut(sb_engine *e, const sb_cut_options *opts, const sb_cut_shape *shapes, uint32_t n_shapes, uint8_t *hit /* [max_beams] or NULL */,
                 int64_t *counts /* [SB_CUT_COUNT_WORDS] or NULL */);

/* ---- the beam graph of the whole scene: edge list and CSR adjacency on the device ----
 * After a cut on the device, or frames in which beams broke, which beams are left and who hangs on whom -- without reading three
 * million beams back.  The definition is sb_batch_graph_device's (below), word for word, on what sb_load_buffers would return at
 * that point of the stream: nodes are the particles at particle DATA indices, edges the LISTED beams at beam DATA indices.  A beam
 * is LIVE by sb_bodies' rule: a caller beam slot of the latest upload that neither a delete pass nor a plan-keeping upload has
 * removed; a pending break flag still connects.  A live beam is listed unless SB_GRAPH_SKIP_PENDING is set and its pending break
 * flag is raised (what the next delete pass will leave).  Half-edges, sides and degrees as there.
 *   ends[d]     int32 {a, b}, the particle data indices of the record's particle_pair, at beam data index d < max_beams; {-1, -1}
 *               where d is not a listed beam.  (The caller holds the upload: materials are not exported.)
 *   row_ptr     int64 [max_particles + 1]: the exclusive prefix sum of the degrees over particle data indices; always complete.
 *   nbr         int32 [max_half_edges][2]: {neighbour, beam data index} by particle, inside a particle by ascending beam data
 *               index (a beam from p to p: side 0, then side 1): a unique order, the same bits on every run.  The first
 *               max_half_edges rows of that list are written, {-1, -1} behind the last half-edge; rows at or behind
 *               max_half_edges are not written.  nbr without row_ptr, or with max_half_edges == 0: SB_ERR_INVALID.
 *   counts      int64 [SB_GRAPH_COUNT_WORDS]: 0 listed beams, 1 particles of degree >= 1, 2 the largest degree, 3 the smallest
 *               data index of a particle of that degree (-1: no beam listed).
 * Each output may be NULL; every element of one that is passed is written.  sb_graph_device only ENQUEUES on the engine's stream,
 * reads nothing back and waits for nothing but the one table build after an upload (the shared scene tables of DESIGN.md 5.22 and
 * sb_cut_device's caller-slot rows); it only READS the engine: frame, graph, frame equals frame, frame bit for bit.  sb_graph is
 * the host-copy convenience: the same launches into buffers of the engine's own, copied back; it waits.
 * Errors, before anything touches a device: SB_ERR_INVALID for a NULL handle, a struct_size that is neither 0 nor the struct's,
 * nonzero reserved words, unknown flag bits, ends / nbr not 4-byte or row_ptr / counts not 8-byte aligned, nbr without row_ptr or
 * with max_half_edges == 0, a scene whose beam data indices reach 2^31; SB_ERR_STATE before an upload; SB_ERR_UNSUPPORTED with
 * ranks.  sb_get_info: "graph_kernel_vgprs", "graph_kernel_scratch_bytes", "graph_table_build_us". */
#define SB_GRAPH_SKIP_PENDING 1u             /* a live beam whose break flag is pending is not listed */
#define SB_GRAPH_COUNT_WORDS 4u
typedef struct sb_graph_options {
    uint32_t struct_size;    /* = sizeof(sb_graph_options); 0 or a NULL pointer = all defaults */
    uint32_t flags;          /* SB_GRAPH_SKIP_PENDING */
    uint64_t max_half_edges; /* rows of nbr; 0 with nbr NULL */
    uint32_t reserved[4];
} sb_graph_options;
sb_status sb_graph_device(sb_engine *e, const sb_graph_options *opts, void *device_ends_i32 /* [max_beams][2] or NULL */,
                          void *device_row_ptr_i64 /* [max_particles + 1] or NULL */,
                          void *device_nbr_i32 /* [max_half_edges][2] or NULL; needs row_ptr */,
                          void *device_counts_i64 /* [SB_GRAPH_COUNT_WORDS] or NULL */);
sb_status sb_graph(sb_engine *e, const sb_graph_options *opts, int32_t *ends, int64_t *row_ptr, int32_t *nbr, int64_t *counts);

/* ---- one summary row of the whole scene, reduced on the device ----
 * What a driver asks of a big scene between steps -- is everything still finite, did it leave the box, how much energy is left,
 * did anything break -- without exporting the state.  The row is SB_SUMMARY_WORDS = 24 floats with the meaning of a row of
 * sb_batch_summary_device (below), word for word: counts in words 0 .. 5, means, extremes, the kinetic energy, word 20 = 1
 * ("uploaded"), words 21 .. 23 = 0; a statistic over an empty set is the quiet NaN 0x7FC00000, counts and the energy are 0 then;
 * a FINITE PARTICLE is one whose six floats are finite, a FINITE BEAM a live beam whose strain and stress are finite.
 * counts (optional, NULL = none): 8 x uint64 -- particles, live beam slots, beams removed by a delete pass (or by a plan-keeping
 * upload), break flags pending among the live beam slots, non-finite particles, non-finite live beams, 1 ("uploaded"), 0.  These
 * are exact whatever the size of the scene; row words 0 .. 5 are (float) of the same integers.  "Pending" is one per beam SLOT
 * flagged since the last delete pass (the bits of the reference's delete mask at this point of the stream), not one per copy
 * the engine's layout keeps of a beam.
 * The arithmetic is sb_batch_summary_device's pin, for any capacity: sums in double; leaf i is the value at DATA index i (+0.0
 * where no finite particle / beam lives), i = 0 .. W-1, W the smallest power of two >= max_particles (particle sums) or
 * >= max_beams (the mean strain); the reduction is the stride-halving tree, for h = W/2 .. 1: s[i] += s[i + h] (i < h); the energy
 * leaf is 0.5 * ((double)vx * vx + (double)vy * vy), word 15 the largest such value without the 0.5; a mean is
 * (float)(sum / (double)finite count); energy and word 15 are rounded to float once.  Extremes compare -0.0 below +0.0 at every
 * stage, so which zero they return does not depend on the cut either.  So a row is the same bits on every run, for
 * every way the reduction is cut into launches, and for a scene that also fits an sb_batch it is that batch's row.
 * sb_summary_options.partials moves the cut (how many partial sums per column the launches pass through): 0 = the engine's
 * choice for its capacity, else a power of two in [256, SB_SUMMARY_MAX_PARTIALS] (the scratch buffer is then at most
 * 48 B * max(partials, W / 16): 12 MiB at the cap for capacities up to 2^22).  The result does not depend on it; it exists for tests
 * and timing.  sb_get_info "summary_partials" reports the one the last call used (the particle tree's, when chosen by the engine).
 * sb_summary_device only ENQUEUES on the engine's stream and writes device memory, which must stay valid until that work has
 * run; sb_summary WAITS and copies to the host.  The first summary after an upload builds its tables (data index -> the engine's
 * own order) on the host and waits for the stream once, as the first export does; later ones only enqueue.  Nothing is read
 * back to the host to form the row.  A summary only reads: positions, the spatial hash, the per-tile flags, the hybrid's
 * schedule and the blocked plan stay as they were, and every later result is the one without the call.
 * Errors: SB_ERR_INVALID for a NULL handle, a NULL row, a row that is not 4-byte or counts that are not 8-byte aligned, a
 * struct_size that is neither 0 nor the struct's, partials that is not such a power of two, a nonzero reserved word, a capacity
 * above 2^31 -- all before anything touches a device; SB_ERR_STATE before an upload; SB_ERR_UNSUPPORTED on an engine with ghost
 * zones or peers configured (per-rank rows are not handled). */
#define SB_SUMMARY_WORDS 24u
#define SB_SUMMARY_MAX_PARTIALS 262144u
typedef struct sb_summary_options {
    uint32_t struct_size;    /* = sizeof(sb_summary_options); 0 or a NULL pointer = all defaults */
    uint32_t partials;       /* partial sums per column at the cut; 0 = the engine's choice */
    uint32_t reserved[6];    /* zero */
} sb_summary_options;
sb_status sb_summary_device(sb_engine *e, const sb_summary_options *opts, void *device_row_f32 /* [SB_SUMMARY_WORDS] float */,
                            void *device_counts_u64 /* [8] uint64 or NULL */);
sb_status sb_summary(sb_engine *e, const sb_summary_options *opts, float *row /* [SB_SUMMARY_WORDS] */, uint64_t *counts /* [8] or NULL */);

/* ---- the connected bodies of the whole scene, labelled on the device ----
 * Is it still one piece, how many fragments, which is the largest -- without reading the scene back for a union-find on the host.
 * The definition is sb_batch_bodies_device's (below), word for word: a BODY is a connected component of the graph whose nodes are
 * the scene's particles and whose edges are its LIVE beams -- the caller's beam slots of the latest upload that neither a delete
 * pass nor a plan-keeping upload that removed beams has removed (the "removed" of sb_load_buffers and of sb_summary's counts).
 * A beam whose break flag is pending still connects.  Everything is indexed by particle DATA index (the rows of
 * sb_read_state_device):
 * labels [max_particles] int32: at index i the smallest data index of the body of particle i, -1 where no particle lives --
 *     for every index up to max_particles; what torch.index_add_ takes for any statistic per body;
 * sizes  [max_particles][2] int32: {particles, live beams} of the body labelled l in row l, {0, 0} in every other row;
 * counts [SB_BODY_WORDS] int64 (like sb_summary's exact counts): bodies, particles of the largest body, bodies of one particle,
 *     label of the largest body (among bodies of equal size the smallest label); a scene of no particles gives {0, 0, 0, -1}.
 * Each output may be NULL (not all three); every word of a non-NULL output is written.  The outputs are integers and the
 * definition names no schedule: they are identical on every run.
 * sb_bodies_device only ENQUEUES on the engine's stream and writes device memory, which must stay valid until that work has
 * run; nothing is read back to the host to decide anything (a lock-free union-find in global memory: no cooperative launch, no
 * grid-wide barrier, no workgroup waits for another).  sb_bodies WAITS and copies to the host.  The first call after an upload
 * builds its tables on the host and waits for the stream once, as the first summary does; later ones only enqueue.  Which
 * beams are live is read on the device at the call's place in the stream.  The call only reads the engine: positions, the
 * spatial hash, the per-tile flags, the hybrid's schedule, the blocked plan and the pending break flags stay as they were.
 * Errors: SB_ERR_INVALID for a NULL handle, three NULL outputs, labels or sizes that are not 4-byte or counts that are not
 * 8-byte aligned, a struct_size that is neither 0 nor the struct's, a nonzero reserved word, a capacity above 2^31 -- all
 * before anything touches a device; SB_ERR_STATE before an upload; SB_ERR_UNSUPPORTED on an engine with ghost zones or peers
 * configured (bodies across ranks are not handled). */
#define SB_BODY_WORDS 4u
typedef struct sb_bodies_options {
    uint32_t struct_size;    /* = sizeof(sb_bodies_options); 0 or a NULL pointer = all defaults */
    uint32_t reserved[7];    /* zero */
} sb_bodies_options;
sb_status sb_bodies_device(sb_engine *e, const sb_bodies_options *opts, void *device_labels_i32 /* [max_particles] int32 or NULL */,
                           void *device_sizes_i32 /* [max_particles][2] int32 or NULL */,
                           void *device_counts_i64 /* [SB_BODY_WORDS] int64 or NULL */);
sb_status sb_bodies(sb_engine *e, const sb_bodies_options *opts, int32_t *labels, int32_t *sizes, int64_t *counts);

/* ---- particle and wall contacts of the whole scene, found on the device ----
 * Who touches whom, and who touches a wall -- without reading the scene back for a grid on the host.  The definition is
 * sb_batch_contacts_device's (below), word for word, for the one scene: particles are named by DATA index (the rows of
 * sb_read_state_device), coordinates are the current particle records at the call's place in the stream, and two distinct
 * particles i, j TOUCH iff dist == 0 or dist < particle_radius * 2, dist = length(xj - xi, yj - yi) in float -- the step's own
 * test, so a pair exactly 2r apart is absent and one an ulp closer is present; a NaN or infinite distance is no contact.  The
 * result depends on the positions alone: not on collision_mode, not on the path.  Wall bits are SB_BATCH_WALL_LEFT / _RIGHT /
 * _LOW / _HIGH with lo = particle_radius, hi = bounds_size - particle_radius in float, compared with <= / >=; a NaN sets none.
 * labels [max_particles] int32 or NULL: any partition of the particles (sb_bodies_device's labels, say); only ever compared.
 * touch  [max_particles][SB_CONTACT_WORDS] int32: per data index {partners, partners of another label (-1 without labels), wall
 *     bits, smallest partner (-1: none)}; {0, 0 or -1, 0, -1} where no particle lives, for every index up to max_particles;
 * pairs  [max_pairs][2] int32: the touching pairs {i, j}, i < j, in ascending (i, j) order, the first max_pairs of them, {-1, -1}
 *     behind the last; with SB_CONTACTS_OTHER_BODY only pairs whose labels differ, order and truncation the same;
 * counts [SB_CONTACT_COUNT_WORDS] int64 (a dense scene exceeds 2^31 pairs): touching pairs (the true number, whatever max_pairs
 *     is), pairs of different labels (-1 without labels), particles on a wall, particles that touch another.
 * Each output may be NULL (not all three); every word of a non-NULL output is written.  Everything behind the float test is
 * integers: the outputs are identical on every run.
 * sb_contacts_device only ENQUEUES on the engine's stream and reads / writes device memory, which must stay valid until that
 * work has run; nothing is read back to decide anything, and no workgroup waits for another (a counting sort by cell in global
 * memory).  sb_contacts WAITS and copies to / from the host.  The first call after an upload builds its table on the host and
 * waits for the stream once; later ones only enqueue.  The call only reads the engine: positions, the spatial hash and its
 * decision state, the per-tile flags, the hybrid's schedule and the blocked plan stay as they were.  Cost: the sum over the
 * particles of the population of their 3 x 3 cells (cells at least 2r (1 + 1/64) wide over [0, bounds]^2, at most about eight a
 * particle); a scene crowded into one cell is quadratic, as it is in the step.
 * Errors: SB_ERR_INVALID for a NULL handle, a struct_size that is neither 0 nor the struct's, an unknown flag bit, a nonzero
 * reserved word, SB_CONTACTS_OTHER_BODY without labels, three NULL outputs, max_pairs > 0 with NULL pairs, labels, touch or pairs
 * that are not 4-byte or counts that are not 8-byte aligned, max_pairs above 2^31 -- all before anything touches a device;
 * SB_ERR_STATE before an upload; SB_ERR_UNSUPPORTED on an engine with ghost zones or peers configured, and where the cell side
 * is no ordinary number (a radius or bounds that are zero, NaN, infinite, beyond 2^+-60) in a scene of more than 4096 particles
 * (at or below 4096 every pair is tested, as the batch does). */
#define SB_CONTACT_WORDS 4u            /* words of a touch row (SB_BATCH_CONTACT_WORDS) */
#define SB_CONTACT_COUNT_WORDS 4u      /* int64 words of counts */
#define SB_CONTACTS_OTHER_BODY 1u      /* the pair list holds only pairs whose particles carry different labels */
typedef struct sb_contacts_options {
    uint32_t struct_size;    /* = sizeof(sb_contacts_options); 0 or a NULL pointer = all defaults: no flags, max_pairs 0 */
    uint32_t flags;          /* SB_CONTACTS_OTHER_BODY */
    uint64_t max_pairs;      /* rows of `pairs`; 0: no list */
    uint32_t reserved[4];    /* zero */
} sb_contacts_options;
sb_status sb_contacts_device(sb_engine *e, const sb_contacts_options *opts, const void *device_labels_i32 /* [max_particles] or NULL */,
                             void *device_touch_i32 /* [max_particles][SB_CONTACT_WORDS] or NULL */,
                             void *device_pairs_i32 /* [max_pairs][2] or NULL */,
                             void *device_counts_i64 /* [SB_CONTACT_COUNT_WORDS] or NULL */);
sb_status sb_contacts(sb_engine *e, const sb_contacts_options *opts, const int32_t *labels, int32_t *touch, int32_t *pairs, int64_t *counts);

/* ---- statistics per body of the whole scene, reproducible bit for bit, on the device ----
 * "Follow the largest fragment", "where did the piece that broke off go", "how fast does each piece move" -- one row of
 * SB_BODY_SUMMARY_WORDS floats per GROUP of particles, without exporting the state.  The definition is
 * sb_batch_body_summary_device's (below), word for word, for the one scene:
 * Groups: labels[i] is read at every particle DATA index i at which a particle lives (never elsewhere).  A value g with
 *   0 <= g < max_particles puts particle i into group g; any other value (-1, negative, too large) into no group.  labels == NULL
 *   means the engine's own bodies: the call first runs sb_bodies_device's labelling into memory of the engine's, on the same stream,
 *   and nothing waits.  Any partition will do (limbs, stripes): nothing assumes connectivity.  A LIVE beam -- sb_bodies' sense: a
 *   caller's beam slot of the latest upload that neither a delete pass nor a plan-keeping upload removed -- belongs to group g iff
 *   BOTH its endpoints are in g; with body labels that is every live beam.  Pending flags (one per beam SLOT flagged since the last
 *   delete pass) and FINITE (a particle whose six floats are finite, a live beam whose strain and stress are) are sb_summary's.
 * Ranking: the non-empty groups are ranked by particles descending, then label ascending (the key by which sb_bodies names the
 *   largest body).  rows[k] is the group of rank k, k < max_rows; rows behind the last group are the EMPTY ROW.  rank[i] is the
 *   rank of particle i's group, however large -- a value >= max_rows means that its row was cut; -1 marks a data index that holds
 *   no particle, or a particle in no group, for every index up to max_particles.  Every word of a non-NULL output is written.
 * Row (words 4 .. 18 mean what they mean in a row of sb_summary_device, restricted to the group):
 *    0  particles of the group (finite or not)       1  live beams of the group
 *    2  the label                                    3  break flags pending among the group's live beam slots
 *    4  particles of the group that are not finite   5  live beams of the group that are not finite
 *    6, 7  mean position x, y                        8, 9  mean velocity x, y           (over the group's finite particles)
 *   10 .. 13  min x, min y, max x, max y             (over the group's finite particles)
 *   14  kinetic energy, the sum of 0.5 (vx^2 + vy^2)    15  max of vx^2 + vy^2          (over the group's finite particles)
 *   16, 17, 18  max strain, max stress, min stress   (over the group's finite beams)
 *   19  angular momentum about the origin, the sum of x vy - y vx                       (over the group's finite particles)
 *   20 .. 23  0
 * Over an empty set a mean or an extreme is the quiet NaN 0x7FC00000; counts, word 14 and word 19 are 0.  The EMPTY ROW: words
 * 0, 1, 3, 4, 5, 14, 19 .. 23 are 0, word 2 is -1, the others NaN.  A scene without particles gives empty rows and rank -1.
 * Words 0 .. 5 are (float) of integers, and an engine can exceed 2^24: rows_i64[k] holds them exactly, SB_BODY_SUMMARY_COUNT_WORDS
 * int64 per row -- particles, live beams, label, pending flags, non-finite particles, non-finite beams, finite particles, 0; the
 * empty row is {0, 0, -1, 0, 0, 0, 0, 0}.
 * The sums are pinned, and the pin is sb_summary's: the sum of a group is what that call's tree gives for a scene that holds only
 * the group's finite particles at their data indices -- in double; leaf i is the value at DATA index i if particle i is finite and
 * in the group, else +0.0; i = 0 .. W-1, W the smallest power of two >= max_particles; for h = W/2 .. 1: s[i] += s[i + h].  The
 * energy leaf is 0.5 * ((double)vx * vx + (double)vy * vy), the candidate of word 15 the same without the 0.5; the
 * angular-momentum leaf is (double)x * vy - (double)y * vx (both products are exact in double: one rounding).  A mean is
 * (float)(sum / (double)finite_count); words 14 and 19 are rounded to float once.  ONE addition to the pin: a sum that is zero is
 * written as +0.0 (the masked tree gives that in every case but a group that fills all W leaves with -0.0).  Extremes compare
 * sb_summary's ordered integer keys from the first comparison on: -0.0 sorts below +0.0, and which zero comes back does not
 * depend on the schedule.  So a row is the same bits on every run.
 * Consequences: for a scene that is ONE body, row 0's words 0, 1, 3 .. 18 equal sb_summary_device's words by their bits; for a
 * scene that also fits an sb_batch the rows are sb_batch_body_summary_device's, every word by its bits.
 * sb_body_summary_device only ENQUEUES on the engine's stream and reads / writes device memory, which must stay valid until that
 * work has run; nothing is read back to decide anything and no workgroup waits for another (a stable radix sort of the members
 * by label and a segmented tree in global memory, one launch per stage and level; the number of groups is read on the device).
 * sb_body_summary WAITS and copies to / from the host.  The first call after an upload builds its tables on the host and waits
 * for the stream once; later ones only enqueue.  Which beams are live is read on the device at the call's place in the stream.
 * The call only reads the engine.  Scratch grows on demand: 137 bytes per data index up to the highest in use, rounded up to a
 * power of two, and 4 bytes per particle of capacity where the labels are the engine's own (sb_get_info
 * "body_summary_scratch_bytes": what the calls so far hold on the device, with the call's two tables: 4 bytes per data index
 * in use and 16 bytes per caller beam slot).
 * sb_body_summary_options.max_rows: 1 .. max_particles; a NULL pointer or struct_size 0 = SB_BODY_SUMMARY_DEFAULT_ROWS rows (at
 * most max_particles).
 * Errors: SB_ERR_INVALID for a NULL handle, three NULL outputs, max_rows of 0 or above max_particles (so also rows non-NULL with
 * max_rows == 0), labels, rows or rank that are not 4-byte or rows_i64 that is not 8-byte aligned, a struct_size that is neither 0
 * nor the struct's, a nonzero reserved word, a capacity above 2^31 -- all before anything touches a device; SB_ERR_STATE before
 * an upload; SB_ERR_UNSUPPORTED on an engine with ghost zones or peers configured (bodies across ranks are not handled). */
#define SB_BODY_SUMMARY_WORDS 24u          /* floats of a row (SB_BATCH_BODY_SUMMARY_WORDS) */
#define SB_BODY_SUMMARY_COUNT_WORDS 8u     /* int64 words of a row of rows_i64 */
#define SB_BODY_SUMMARY_DEFAULT_ROWS 8u
typedef struct sb_body_summary_options {
    uint32_t struct_size;    /* = sizeof(sb_body_summary_options); 0 or a NULL pointer = all defaults */
    uint32_t reserved[5];    /* zero */
    uint64_t max_rows;       /* rows of `rows` and `rows_i64`: 1 .. max_particles */
} sb_body_summary_options;
sb_status sb_body_summary_device(sb_engine *e, const sb_body_summary_options *opts,
        const void *device_labels_i32 /* [max_particles] or NULL */,
        void *device_rows_f32         /* [max_rows][SB_BODY_SUMMARY_WORDS] float or NULL */,
        void *device_rows_i64         /* [max_rows][SB_BODY_SUMMARY_COUNT_WORDS] int64 or NULL */,
        void *device_rank_i32         /* [max_particles] int32 or NULL */);
sb_status sb_body_summary(sb_engine *e, const sb_body_summary_options *opts, const int32_t *labels, float *rows, int64_t *rows_i64,
                          int32_t *rank);

/* ---- batched small scenes: N independent scenes, one workgroup per scene, one launch per frame ----
 * A second object beside sb_engine, for the user who steps thousands of copies of a SMALL scene (a controller, an RL loop):
 * every scene is a full scene of the reference -- its own particles, beams, mapping, counts, physics constants and user input --
 * and all of them advance in ONE launch per frame, each in the LDS of its own workgroup.  The arithmetic is sb_engine's
 * (the same device functions), so every scene's bytes are those of an sb_engine / of the reference's all-pairs loop.
 * An sb_batch never touches an sb_engine.
 *   Limits: per scene at most SB_BATCH_MAX_PARTICLES particles and SB_BATCH_MAX_BEAMS beams (what one workgroup holds).
 *   When do calls return?  sb_batch_frame / _step / _delete_pass / _reset_device / _write_user_input[_device] /
 *     _set_physics_constants / _read_state_device / _write_particles_device / _fork_device / _checkpoint_device /
 *     _write_beams_device / _add_beams_device / _add_particles_device / _summary_device / _rollout_device / _bodies_device / _contacts_device / _graph_device / _raycast_device / _nearest_device / _forces_device only ENQUEUE on the batch's stream (device buffers must stay valid until that work has run); sb_batch_write_scene, sb_batch_load_scene and sb_batch_sync WAIT for it.
 *     sb_batch_render_device only ENQUEUES (its device buffer must stay valid likewise); sb_batch_render_scene WAITS.
 *   Errors: every call returns an sb_status; sb_batch_last_error(b) gives the message (b == NULL: the last failed
 *     sb_batch_create of the calling thread).  Options are checked BEFORE a device is looked for. */
#define SB_BATCH_MAX_PARTICLES 1024
#define SB_BATCH_MAX_BEAMS 4096
typedef struct sb_batch sb_batch;
typedef struct sb_batch_options {
    uint32_t struct_size;    /* = sizeof(sb_batch_options) */
    uint32_t n_scenes;       /* >= 1 */
    float bounds_size;       /* as sb_options */
    float particle_radius;
    uint32_t subticks;       /* rounded UP to even; time_step = 1/subticks */
    uint32_t max_particles;  /* capacity PER SCENE, 1 .. SB_BATCH_MAX_PARTICLES */
    uint32_t max_beams;      /* capacity PER SCENE, 0 .. SB_BATCH_MAX_BEAMS */
    uint32_t layout;         /* SB_LAYOUT_* of the host buffers of sb_batch_write_scene / sb_batch_load_scene */
    uint32_t collision_mode; /* SB_COLLIDE_OFF; SB_COLLIDE_ALLPAIRS: the reference's loop over all slots in ascending order
                              * (compute.wgsl:144-170); SB_COLLIDE_GRID (the default): scenes of at least grid_min_particles
                              * particles bin their particles into a uniform cell grid in LDS every substep and test only the
                              * 3 x 3 cells around each particle, applying the contacts in the same ascending slot order -- the
                              * same bits as SB_COLLIDE_ALLPAIRS, O(P) instead of O(P^2); smaller scenes, and any substep in which
                              * a cell holds more than "contact_cell_capacity" particles, run the loop */
    int32_t device_ordinal;
    uint32_t grid_min_particles; /* SB_COLLIDE_GRID: 0 = the build's default (the measured break-even, sb_batch_get_info
                              * "grid_min_particles"), n = scenes of at least n particles (1 .. SB_BATCH_MAX_PARTICLES) use the
                              * cells, 0xFFFFFFFF = never.  Anything else is SB_ERR_INVALID.  Ignored by the other modes.
                              * (carved from `reserved`: zero, as sb_batch_default_options always left it, is the default) */
    uint32_t reserved[5];
} sb_batch_options;

/* reference defaults (bounds 1000, radius 10, subticks 64, v1, collisions on, device 0), one scene at the capacity limit */
void sb_batch_default_options(sb_batch_options *opts);
sb_status sb_batch_create(const sb_batch_options *opts, sb_batch **out);
sb_status sb_batch_destroy(sb_batch *b);

/* ONE scene in the four host buffers of sb_write_buffers (full per-scene capacity, the same validation) into scenes
 * first .. first+count-1; count = n_scenes replicates it over the batch.  The upload also becomes those scenes' RESET state.
 * Scenes never uploaded hold zero particles and step as no-ops. */
sb_status sb_batch_write_scene(sb_batch *b, uint32_t first, uint32_t count, const void *metadata, size_t metadata_bytes,
                               const void *mapping, size_t mapping_bytes, const void *particles, size_t particles_bytes,
                               const void *beams, size_t beams_bytes);
/* the 32 bytes at metadata offset 80 of EVERY scene from host memory ... */
sb_status sb_batch_write_user_input(sb_batch *b, const void *bytes32);
/* ... or n_scenes x 32 bytes from device memory, scene after scene (per-scene actions straight from a tensor) */
sb_status sb_batch_write_user_input_device(sb_batch *b, const void *device_bytes);
/* the 8 floats at metadata offset 48 of scenes first .. first+count-1 */
sb_status sb_batch_set_physics_constants(sb_batch *b, uint32_t first, uint32_t count, const float constants8[8]);

/* every scene: n_frames x (subticks substeps, then one delete pass), the user input held constant; one launch per frame */
sb_status sb_batch_frame(sb_batch *b, uint32_t n_frames);
/* n substeps without a delete pass (any n; one launch), and the delete pass on its own */
sb_status sb_batch_step(sb_batch *b, uint32_t n_substeps);
sb_status sb_batch_delete_pass(sb_batch *b);

/* scenes whose byte in device_mask_u8[n_scenes] is nonzero go back to their reset state: that of their latest upload, or of a
 * later sb_batch_checkpoint_device / sb_batch_fork_device (particles, beam state, beam mapping, counts, pending break flags);
 * user input and physics constants stay.  NULL = all scenes. */
sb_status sb_batch_reset_device(sb_batch *b, const void *device_mask_u8);

/* the layouts of sb_read_state_device / sb_write_particles_device with a leading scene dimension: particles
 * [n_scenes][max_particles] x 24 B at each particle's DATA index, beams [n_scenes][max_beams] x 16 B {target_length,
 * last_length, strain, stress}, beam_alive [n_scenes][max_beams] bytes.  Rows of no particle / beam of a scene's latest upload
 * are not written (not read).  Any pointer of the export may be NULL.  Pointers must be 4-byte aligned. */
sb_status sb_batch_read_state_device(sb_batch *b, void *device_particles, void *device_beams, void *device_beam_alive);
sb_status sb_batch_write_particles_device(sb_batch *b, const void *device_particles);

/* ---- fork, checkpoint, beam import: the planner's and the policy's moves between frames, on the device ----
 * All three only ENQUEUE on the batch's stream (device buffers must stay valid until that work has run).  Their argument errors
 * -- a NULL handle, a NULL or misaligned (not 4-byte) pointer where one is required, unknown flag / field bits -- are
 * SB_ERR_INVALID and are checked before anything touches a device.
 *
 * sb_batch_fork_device -- device_src_u32[n_scenes]: scene i becomes a copy of scene src[i].
 *   Snapshot: every source is read as it was when the call's work began, so a permutation, a swap, or a broadcast from a scene
 *     that is itself overwritten are well defined.  (Two launches through a staging set of blobs that the first fork allocates
 *     and the batch keeps: sb_batch_get_info "fork_staging_bytes"; 0 before the first fork.)
 *   src[i] == i and src[i] == SB_BATCH_FORK_KEEP leave scene i byte for byte as it was.  Any other entry >= n_scenes leaves
 *     scene i untouched as well, is never used as an index, and is counted in sb_batch_get_info "fork_bad_sources" (all forks
 *     so far; that key WAITS for the stream).
 *   Copied: the constant blob (topology, materials, the "holds a particle / beam of the upload" bytes), the current state
 *     (particle records, beam state, beam mapping, pending break flags, which beams were removed) and the metadata words that
 *     describe the scene (the reference's counts and indices, words 0 .. 11, and "uploaded").  The destination KEEPS its 8 user
 *     input words (the action) and, unless SB_BATCH_FORK_CONSTANTS is set, its 8 physics constants, as a reset does.
 *   "Latest upload" in sb_batch_read_state_device, sb_batch_write_particles_device and sb_batch_write_beams_device means, for
 *     a forked scene, its SOURCE's upload: the rows those calls touch travel with the constant blob.
 *   Reset state: a reset image only makes sense beside the constant blob it was made for, so a fork never leaves the
 *     destination's old one behind.  Without SB_BATCH_FORK_AS_RESET the destination also receives the source's reset state: a
 *     later reset takes it where a reset would take the source (the source's upload, or its checkpoint).  With
 *     SB_BATCH_FORK_AS_RESET the forked state itself becomes the destination's reset state.  Either way a later reset is well
 *     defined and fault-free.  (Scenes the fork leaves untouched keep their reset state under both flags.)
 *   A source that was never uploaded makes the destination a never-uploaded scene: it steps as a no-op, renders black, and
 *     sb_batch_load_scene returns SB_ERR_STATE for it. */
#define SB_BATCH_FORK_KEEP 0xFFFFFFFFu
#define SB_BATCH_FORK_CONSTANTS 1u /* the source's 8 physics constants come along */
#define SB_BATCH_FORK_AS_RESET 2u  /* the forked state becomes the destination's reset state */
sb_status sb_batch_fork_device(sb_batch *b, const void *device_src_u32, uint32_t flags);

/* the inverse of sb_batch_reset_device: scenes whose byte in device_mask_u8[n_scenes] is nonzero (NULL = all scenes) make their
 * CURRENT state their reset state -- particles, beam state, beam mapping, live-beam count, pending break flags, which beams were
 * removed.  Scenes never uploaded are skipped.  A later reset returns to exactly these bytes. */
sb_status sb_batch_checkpoint_device(sb_batch *b, const void *device_mask_u8);

/* the counterpart of sb_batch_write_particles_device for beams: device_beams in sb_batch_read_state_device's beam layout,
 * [n_scenes][max_beams] x 16 B {target_length, last_length, strain, stress} at DATA indices.  `fields` selects what is written:
 * SB_BATCH_BEAM_TARGET_LENGTH and / or SB_BATCH_BEAM_LAST_LENGTH (zero or any other bit: SB_ERR_INVALID); strain and stress are
 * the step's outputs and are never imported.  Only rows of beams of the scene's latest upload are read; a removed beam's row is
 * written but inert.  Counts, mappings, "removed" bytes and pending break flags are untouched.  Every later result is the one
 * the batch would compute had those floats been these bytes all along. */
#define SB_BATCH_BEAM_TARGET_LENGTH 1u
#define SB_BATCH_BEAM_LAST_LENGTH 2u
sb_status sb_batch_write_beams_device(sb_batch *b, const void *device_beams, uint32_t fields);

/* sb_batch_cut_device -- the planner's "tear it here": sb_cut_device (above) for every scene in ONE launch.  device_shapes is
 * [n_scenes][k] sb_cut_shape, k <= SB_CUT_MAX_SHAPES: scene i is cut by its own k shapes.  The predicate, "hit", "live" (the
 * scene's live beam slots) and the four counts are sb_cut_device's, word for word; the counts are int32 here,
 * device_counts_i32 [n_scenes][SB_CUT_COUNT_WORDS].  device_hit_u8 [n_scenes][max_beams]: 1 / 0 at beam DATA indices, zero-filled
 * over max_beams for every scene.  flags: SB_CUT_DRY_RUN.  A hit beam's pending break flag is raised: the scene's next frame (or
 * rollout) removes it in its delete pass, a reset undoes it, a fork copies it, a checkpoint keeps it.  A scene whose k shapes are
 * all SB_CUT_NONE, or that was never uploaded, is left untouched bit for bit; its counts row and its hit row are still written.
 * Only ENQUEUES on the batch's stream.  Either output may be NULL.  Errors, before anything touches a device: SB_ERR_INVALID for
 * a NULL handle, unknown flag bits, k > SB_CUT_MAX_SHAPES, NULL shapes with k > 0, a shape or counts pointer that is not
 * 4-byte aligned.  sb_batch_get_info: "cut_kernel_vgprs", "cut_kernel_scratch_bytes". */
sb_status sb_batch_cut_device(sb_batch *b, uint32_t flags, const void *device_shapes /* [n_scenes][k] sb_cut_shape */, uint32_t k,
                              void *device_hit_u8 /* [n_scenes][max_beams] or NULL */,
                              void *device_counts_i32 /* [n_scenes][SB_CUT_COUNT_WORDS] int32 or NULL */);

/* ---- adding beams on the device ("welds"), the inverse of a cut ----
 * sb_batch_add_beams_device -- the planner's "glue these two": every scene gets its own k rows of new beams in ONE launch.
 * device_rows is [n_scenes][k] sb_batch_new_beam, k <= SB_BATCH_ADD_MAX; contacts' pair list holds exactly the (a, b) a row wants.
 *
 * DEFINITION.  Scene i processes its k rows in row order.  Row j is decided in four steps.
 * 1. Empty.  a < 0 gives EMPTY.  The row is not counted.
 * 2. Invalid.  The row is INVALID if any of these hold: the scene was never uploaded; a or b is >= max_particles; a == b;
 *    either endpoint is not the data index of a particle slot < P; reserved != 0; the resolved length is not a finite number
 *    > 0.  The length is resolved as follows.  The current distance is sb_length(pb.x - pa.x, pb.y - pa.y) on the current
 *    particle records; these are the beam phase's own expressions.  With LENGTH_CURRENT the resolved length is the current
 *    distance.  Otherwise it is the row's length.  A distance of 0 or NaN under LENGTH_CURRENT is therefore INVALID.  spring,
 *    damp, yield_strain and strain_break_limit are taken verbatim, as an upload takes them.
 * 3. Joined.  This step applies only with SKIP_JOINED.  The row is JOINED in either of these cases: a live beam slot
 *    (< beam_i_c; a pending break flag still joins) connects the unordered pair {a, b}; an earlier row of this call, not EMPTY,
 *    INVALID or JOINED, names the same unordered pair.
 * 4. Room.  The rows that survive are the candidates.  Their rank r is the number of candidates before them.  A candidate is
 *    added when beam_i_c + r < max_beams and there is an r-th free beam data index.  Otherwise it is FULL.  Room is first come,
 *    first served, so the duplicate rule above cannot depend on it.
 * Free data index.  A beam data index d is free when balive[d] == 0 in the CURRENT state blob AND in the RESET state blob
 * (balive[d] == 1 iff a live slot of that state's beam mapping names d: DESIGN.md 5.24).  No live slot of either state's mapping
 * names such an index, so its constant rows may be rewritten without corrupting a later reset.  An index a delete pass freed
 * becomes reusable once a checkpoint has made that removal part of the reset state.  An addition that a reset undoes frees its
 * index again: episodes of weld, reset, weld do not leak capacity.
 * What the r-th added beam writes.  It takes the r-th smallest free data index d and beam slot beam_i_c + r.  Constant blob:
 * endpoint SLOTS of a and b (through the inverse of the particle mapping), the material row {length, spring, damp, yield, limit,
 * 1 / length} with one IEEE divide, the upload's own, and "holds a beam of the upload" = 1.  State blob: the beam's state
 * {target_length = length, last_length = current distance, strain 0, stress 0}, beam mapping [slot] = d, alive [d] = 1, the slot's
 * pending break bit CLEARED.  After all rows metadata.beam_i_c += added.  The reset state and its beam count are untouched.
 * Outputs.  result[j] is d for an added row, else the code.  counts = {added, invalid, joined, full}.  With DRY_RUN, result and
 * counts are the real call's and nothing else is written.
 *
 * CONSEQUENCES.  Every later launch sees the beam as if it had been uploaded: frame, reports, render, read_state_device,
 * write_beams_device, load_scene, cut and fork.  checkpoint keeps it and reset removes it.  After such a reset the index reads
 * "of the upload" = 1, alive = 0: sb_batch_summary_device's word 2 counts it as "removed", like a beam a delete pass removed;
 * reusing an index lowers that word by one.  A scene with no candidate row (or none that finds room) is left bit for bit as it was.
 *
 * Only ENQUEUES on the batch's stream.  Either output may be NULL.  Errors, before anything touches a device: SB_ERR_INVALID for a
 * NULL handle, unknown flag bits, k > SB_BATCH_ADD_MAX, NULL rows with k > 0, a pointer that is not 4-byte aligned.  k == 0 is
 * SB_OK: the counts rows are still written, as zeros.  sb_batch_get_info: "add_beams_kernel_vgprs",
 * "add_beams_kernel_scratch_bytes". */
typedef struct sb_batch_new_beam { /* 32 bytes */
    int32_t a, b;            /* particle DATA indices (what state_tensors / contacts use); a < 0: empty row */
    float length;            /* rest length; see SB_BATCH_ADD_LENGTH_CURRENT */
    float spring, damp, yield_strain, strain_break_limit;
    uint32_t reserved;       /* 0 */
} sb_batch_new_beam;
#define SB_BATCH_ADD_MAX 64u            /* rows per scene and call */
#define SB_BATCH_ADD_DRY_RUN 1u
#define SB_BATCH_ADD_LENGTH_CURRENT 2u  /* length := the endpoints' current distance */
#define SB_BATCH_ADD_SKIP_JOINED 4u
#define SB_BATCH_ADD_EMPTY (-1)
#define SB_BATCH_ADD_INVALID (-2)
#define SB_BATCH_ADD_JOINED (-3)
#define SB_BATCH_ADD_FULL (-4)
#define SB_BATCH_ADD_COUNT_WORDS 4u     /* added, invalid, joined, full */
sb_status sb_batch_add_beams_device(sb_batch *b, uint32_t flags, const void *device_rows /* [n_scenes][k] sb_batch_new_beam */, uint32_t k,
                                    void *device_result_i32 /* [n_scenes][k] int32 or NULL */,
                                    void *device_counts_i32 /* [n_scenes][SB_BATCH_ADD_COUNT_WORDS] int32 or NULL */);

/* ---- adding particles on the device ("spawns"), undone by a reset ----
 * sb_batch_add_particles_device -- the planner's "throw a ball at it": every scene gets its own k rows of new particles in ONE
 * launch.  device_rows is [n_scenes][k] sb_batch_new_particle, k <= SB_BATCH_ADD_MAX.  The result names the DATA indices the new
 * particles got: what a row of sb_batch_add_beams_device wants as a or b, so spawn -> weld makes a whole body in two launches.
 *
 * DEFINITION.  Scene i processes its k rows in row order.  P is metadata.particle_i_c as the call finds it.  Row j is decided in
 * four steps.
 * 1. Empty.  tag < 0 gives EMPTY.  The row is not counted.  (tag >= 0 is the caller's own: it is not stored.)
 * 2. Invalid.  The row is INVALID if any of these hold: the scene was never uploaded; reserved != 0; x or y is not finite.
 *    vx, vy, ax and ay are taken verbatim, non-finite values included, as an upload takes them.  A position outside the box is
 *    legal: the step clamps it.
 * 3. Blocked.  This step applies only with SKIP_TOUCHING.  "Touches" is the contact test of the step and of
 *    sb_batch_contacts_device, in the same float expressions, with the batch's particle_radius: dist = sqrt(dx * dx + dy * dy),
 *    touching when dist == 0 or dist < 2 * radius.  Let E(j) mean: row j touches the current position of a particle slot < P.
 *    Row j is BLOCKED if E(j) holds.  Row j is also BLOCKED if it touches an earlier row i that is not EMPTY, not INVALID and not
 *    E(i) -- whether or not row i was itself blocked by a still earlier row, or found no room.  The rule needs no serial pass and
 *    does not depend on room; it is deliberately conservative.
 * 4. Room.  The rows that survive are the candidates.  Their rank r is the number of candidates before them.  A candidate is
 *    added when P + r < max_particles and there is an r-th free particle data index.  Otherwise it is FULL.
 * Free data index.  A particle data index d is free when "holds a particle" [d] == 0 in the constant blob ("holds a particle" [d]
 * == 1 iff a slot < P of the scene's particle mapping names d: DESIGN.md 5.26).
 * What the r-th added particle writes.  It takes the r-th smallest free data index d and particle slot P + r.  Constant blob:
 * particle mapping [P + r] = d, "holds a particle" [d] = 1.  Current state blob: the particle record at d = {x, y, vx, vy, ax, ay}.
 * After all rows metadata.particle_i_c += added.  The reset state and its particle count are untouched, and so is every other
 * metadata word (word 0, particle_v_c, is the constant 3 of the reference's record: nothing the batch reads depends on it).
 * Outputs.  result[j] is d for an added row, else the code.  counts = {added, invalid, blocked, full}.  With DRY_RUN, result and
 * counts are the real call's and nothing else is written.
 *
 * CONSEQUENCES.  Every later launch sees the particle as if it had been uploaded: frame, reports, render, read_state_device,
 * write_particles_device, load_scene, add_beams and fork.  sb_batch_checkpoint_device keeps it (the reset particle count becomes
 * P).  sb_batch_reset_device removes it: the slots from the reset particle count on give their data indices back, and with them
 * goes every beam welded onto them, since such a beam is younger than the reset state.  Episodes of spawn, reset, spawn do not
 * leak capacity.  sb_batch_fork_device copies it, with the source's reset particle count (SB_BATCH_FORK_AS_RESET: the source's P).
 * A scene with no added row is left bit for bit as it was.
 *
 * Only ENQUEUES on the batch's stream.  Either output may be NULL.  Errors, before anything touches a device: SB_ERR_INVALID for a
 * NULL handle, unknown flag bits, k > SB_BATCH_ADD_MAX, NULL rows with k > 0, a pointer that is not 4-byte aligned.  k == 0 is
 * SB_OK: the counts rows are still written, as zeros.  sb_batch_get_info: "add_particles_kernel_vgprs",
 * "add_particles_kernel_scratch_bytes". */
typedef struct sb_batch_new_particle { /* 32 bytes */
    int32_t tag;             /* < 0: empty row */
    float x, y, vx, vy, ax, ay; /* the six floats of a particle record, taken verbatim as an upload takes them */
    uint32_t reserved;       /* 0 */
} sb_batch_new_particle;
#define SB_BATCH_SPAWN_DRY_RUN 1u
#define SB_BATCH_SPAWN_SKIP_TOUCHING 2u
#define SB_BATCH_SPAWN_EMPTY (-1)
#define SB_BATCH_SPAWN_INVALID (-2)
#define SB_BATCH_SPAWN_BLOCKED (-3)
#define SB_BATCH_SPAWN_FULL (-4)
#define SB_BATCH_SPAWN_COUNT_WORDS 4u   /* added, invalid, blocked, full */
sb_status sb_batch_add_particles_device(sb_batch *b, uint32_t flags, const void *device_rows /* [n_scenes][k] sb_batch_new_particle */,
                                        uint32_t k, void *device_result_i32 /* [n_scenes][k] int32 or NULL */,
                                        void *device_counts_i32 /* [n_scenes][SB_BATCH_SPAWN_COUNT_WORDS] int32 or NULL */);

/* ---- per-scene summary rows and multi-frame rollouts on the device ----
 * sb_batch_summary_device -- one row of SB_BATCH_SUMMARY_WORDS floats per scene into device_out_f32[n_scenes][SB_BATCH_SUMMARY_WORDS],
 * in ONE launch: what a done-test or a score reads of a scene without exporting its state.  It only ENQUEUES and only READS the
 * batch: frame, summary, frame equals frame, frame bit for bit, pending break flags included.  Every word of every row is
 * written.  Counts are floats (all <= 4096: exact).  A FINITE PARTICLE is one whose six floats are all finite; a FINITE BEAM is a
 * live beam (of the scene's upload and not removed) whose strain and stress are both finite.
 *    0  particles of the scene                      1  live beam slots (metadata.beam_i_c)
 *    2  beams of the upload that a delete pass has removed
 *    3  break flags pending (set bits among the live beam slots)
 *    4  particles that are not finite               5  live beams that are not finite
 *    6, 7  mean position x, y                       8, 9  mean velocity x, y            (over the finite particles)
 *   10 .. 13  min x, min y, max x, max y            (over the finite particles)
 *   14  kinetic energy, the sum of 0.5 (vx^2 + vy^2)   15  max of vx^2 + vy^2           (over the finite particles)
 *   16, 17, 18  max strain, max stress, min stress  19  mean strain                     (over the finite beams)
 *   20  1 if the scene was ever uploaded (or forked from one that was), else 0          21 .. 23  0
 * A statistic over an empty set (means, extremes) is the quiet NaN 0x7FC00000; counts and the energy are 0 then.  A scene never
 * uploaded gives counts 0, word 20 = 0 and NaN elsewhere.
 * The arithmetic is pinned, so a row is reproducible bit for bit: sums are taken in double; leaf i of a sum is the value at DATA
 * index i (+0.0 where no finite particle / beam lives), i = 0 .. W-1, W the smallest power of two >= max_particles (particle sums)
 * or >= max_beams (beam sums); the reduction is the stride-halving tree, for h = W/2, W/4, .. 1: s[i] += s[i + h] (i < h).  The
 * energy leaf is 0.5 * ((double)vx * vx + (double)vy * vy), the candidate of word 15 the same without the 0.5; a mean is
 * (float)(sum / (double)count); energy and word 15 are rounded to float once, at the end (beyond float's range: +inf).  Extremes
 * are taken in the order of the floats' keys, in which -0.0 lies below +0.0: over both zeros a minimum is -0.0, a maximum +0.0.
 * Errors: SB_ERR_INVALID for a NULL handle, a NULL output, a pointer that is not 4-byte aligned -- before anything touches a device.
 *
 * sb_batch_rollout_device -- n_frames times, in this order: slice t of device_inputs[n_frames][n_scenes][32 B] applied exactly as
 * sb_batch_write_user_input_device would (NULL: the inputs stay as they are); one frame exactly as sb_batch_frame(b, 1); the
 * summary of the state after that frame into slice t of device_summaries[n_frames][n_scenes][SB_BATCH_SUMMARY_WORDS] (NULL: none).
 * A host-side sequence of those launches, enqueued in one call: bit for bit the result of the individual calls; "frames_done" and
 * "substeps_done" advance as they would; afterwards the scenes hold the inputs of the last slice.  n_frames = 0: SB_OK, nothing
 * done.  A pointer that is not 4-byte aligned: SB_ERR_INVALID, before anything touches a device. */
#define SB_BATCH_SUMMARY_WORDS 24u
sb_status sb_batch_summary_device(sb_batch *b, void *device_out_f32 /* [n_scenes][SB_BATCH_SUMMARY_WORDS] float */);
sb_status sb_batch_rollout_device(sb_batch *b, uint32_t n_frames,
                                  const void *device_inputs  /* [n_frames][n_scenes][32 B] or NULL: inputs stay as they are */,
                                  void *device_summaries     /* [n_frames][n_scenes][SB_BATCH_SUMMARY_WORDS] float or NULL */);

/* ---- the connected bodies of every scene, labelled on the device ----
 * sb_batch_bodies_device -- what the breaking of beams did to the bodies, in ONE launch.  A BODY is a connected component of the
 * graph whose nodes are the scene's particles and whose edges are its LIVE beams (the beam slots 0 .. metadata.beam_i_c - 1).  A
 * beam whose break flag is pending is still live and still connects; it stops connecting when a delete pass has removed it,
 * exactly as it stops exerting force.  Every output is indexed by particle DATA index, like sb_batch_read_state_device's rows;
 * any of the three may be NULL (not written), not all of them; every word of a non-NULL output is written.
 *   labels[s][i]  the smallest data index among the particles of the body that particle i belongs to; -1 where data index i holds
 *                 no particle of the scene's upload.  (The definition names no schedule: the bits are the same on every run.)
 *   sizes[s][i]   {particles, live beams} of the body whose label is i; {0, 0} in every other row.  A beam belongs to the body of
 *                 its endpoints.
 *   counts[s]     SB_BATCH_BODY_WORDS words: 0 bodies, 1 particles of the largest body, 2 bodies of exactly one particle,
 *                 3 label of the largest body (of several that large, the smallest label).  A scene of no particles, or one never
 *                 uploaded, gives {0, 0, 0, -1} and labels of -1.
 * labels is what torch.index_add_ needs for a statistic per body; counts[:, 0] is the "still whole" / "torn in two" test.
 * It only ENQUEUES and only READS the batch: frame, bodies, frame equals frame, frame bit for bit.  Integers only.
 * Errors: SB_ERR_INVALID for a NULL handle, for three NULL outputs, for a pointer that is not 4-byte aligned -- before anything
 * touches a device. */
#define SB_BATCH_BODY_WORDS 4u
sb_status sb_batch_bodies_device(sb_batch *b,
                                 void *device_labels_i32  /* [n_scenes][max_particles] int32 or NULL */,
                                 void *device_sizes_i32   /* [n_scenes][max_particles][2] int32 or NULL */,
                                 void *device_counts_i32  /* [n_scenes][SB_BATCH_BODY_WORDS] int32 or NULL */);

/* ---- statistics per body, reproducible bit for bit ----
 * sb_batch_body_summary_device -- one row of SB_BATCH_BODY_SUMMARY_WORDS floats per GROUP of particles of every scene, in ONE
 * launch: "follow the largest fragment", "where did the piece that broke off go", "how fast does each piece move".  It only
 * ENQUEUES on the batch's stream and only READS the batch: frame, body_summary, frame equals frame, frame bit for bit.
 * Groups: labels[s][i] is read at every particle DATA index i of scene s (never at a data index that holds no particle).  A value
 *   g with 0 <= g < max_particles puts particle i into group g; any other value (-1, negative, too large) into no group.  With
 *   the labels sb_batch_bodies_device writes the groups are the bodies, but any partition will do (limbs, stripes): nothing
 *   assumes connectivity.  A live beam (beam slots 0 .. metadata.beam_i_c - 1) belongs to group g iff BOTH its endpoints are in g;
 *   with body labels that is every live beam.
 * Ranking: the non-empty groups of a scene are ranked by particles descending, then label ascending (the key by which
 *   sb_batch_bodies_device names the largest body).  rows[s][k] is the group of rank k, k < max_rows; rows behind the last group
 *   are the EMPTY ROW.  rank[s][i] is the rank of particle i's group, however large -- a value >= max_rows means that its row was
 *   cut; -1 marks a data index that holds no particle, or a particle in no group.  Every word of a non-NULL output is written.
 * Row (words 4 .. 18 mean what they mean in a row of sb_batch_summary_device, restricted to the group):
 *    0  particles of the group (finite or not)       1  live beams of the group
 *    2  the label (<= 1023: exact as a float)        3  break flags pending among the group's live beam slots
 *    4  particles of the group that are not finite   5  live beams of the group that are not finite
 *    6, 7  mean position x, y                        8, 9  mean velocity x, y           (over the group's finite particles)
 *   10 .. 13  min x, min y, max x, max y             (over the group's finite particles)
 *   14  kinetic energy, the sum of 0.5 (vx^2 + vy^2)    15  max of vx^2 + vy^2          (over the group's finite particles)
 *   16, 17, 18  max strain, max stress, min stress   (over the group's finite beams)
 *   19  angular momentum about the origin, the sum of x vy - y vx                       (over the group's finite particles)
 *   20 .. 23  0
 * Over an empty set a mean or an extreme is the quiet NaN 0x7FC00000; counts, word 14 and word 19 are 0.  The EMPTY ROW: words
 * 0, 1, 3, 4, 5, 14, 19 .. 23 are 0, word 2 is -1, the others NaN.  A scene never uploaded, and a scene without particles, give
 * empty rows and rank -1.  (The mean strain is deliberately not in the row: it would need a second pinned tree over up to 4096
 * beam leaves.  The beam words are the order-free ones.)
 * The sums are pinned, and the pin is sb_batch_summary_device's: the sum of a group is what that call's tree gives for a scene
 * that holds only the group's finite particles at their data indices -- in double; leaf i is the value at DATA index i if particle
 * i is finite and in the group, else +0.0; i = 0 .. W-1, W the smallest power of two >= max_particles; for h = W/2 .. 1:
 * s[i] += s[i + h].  The energy leaf is 0.5 * ((double)vx * vx + (double)vy * vy), the candidate of word 15 the same without the
 * 0.5; the angular-momentum leaf is (double)x * vy - (double)y * vx (both products are exact in double: one rounding).  A mean is
 * (float)(sum / (double)finite_count); words 14 and 19 are rounded to float once.  ONE addition to the pin: a sum that is zero is
 * written as +0.0.  The masked tree gives that in every case but one -- a group that fills all W leaves with -0.0, where the tree
 * gives -0.0 and this call still writes +0.0.  Extremes as in sb_batch_summary_device's row (-0.0 below +0.0).
 * Consequence: for a scene that is ONE body, row 0's words 0, 1, 3 .. 18 equal sb_batch_summary_device's words by their bits.
 * Errors: SB_ERR_INVALID for a NULL handle, NULL labels, rows and rank both NULL, max_rows of 0 or above max_particles (so also
 * rows non-NULL with max_rows == 0), a pointer that is not 4-byte aligned -- before anything touches a device. */
#define SB_BATCH_BODY_SUMMARY_WORDS 24u
sb_status sb_batch_body_summary_device(sb_batch *b,
        const void *device_labels_i32 /* [n_scenes][max_particles] int32, required */,
        uint32_t max_rows             /* 1 .. max_particles */,
        void *device_rows_f32         /* [n_scenes][max_rows][SB_BATCH_BODY_SUMMARY_WORDS] float or NULL */,
        void *device_rank_i32         /* [n_scenes][max_particles] int32 or NULL */);

/* ---- the pose of every body against a reference shape, reproducible bit for bit ----
 * sb_batch_pose_device -- how is every GROUP of particles of every scene turned, how fast does it spin, how far is it bent out of
 * shape?  One row of SB_BATCH_POSE_WORDS floats and one of SB_BATCH_POSE_MOMENT_WORDS doubles per group, in ONE launch: the
 * centroids and the moments of the 2-D shape-matching fit of the group's current positions against a REFERENCE configuration.  It
 * only ENQUEUES on the batch's stream and only READS the batch: frame, pose, frame equals frame, frame bit for bit.
 * Groups, ranking, rank, empty rows: sb_batch_body_summary_device's, word for word.  labels[s][i] is read at every particle DATA
 *   index i of scene s (never at a data index that holds no particle); a value g with 0 <= g < max_particles puts particle i into
 *   group g, any other value into no group.  The non-empty groups of a scene are ranked by particles descending, then label
 *   ascending: rows[s][k] and moments[s][k] belong to the group of rank k -- the group of row k of sb_batch_body_summary_device
 *   for the same labels --, rows behind the last group are the EMPTY ROW; rank[s][i] is the rank of particle i's group, however
 *   large, -1 at a data index that holds no particle or a particle in no group.  Every word of a non-NULL output is written.
 * Reference: with device_ref_f32, the reference position {X, Y} of particle i is ref[s][i], at its DATA index.  With NULL it is the
 *   x and y of particle i's record in the scene's RESET state (its latest upload, sb_batch_checkpoint_device or
 *   sb_batch_fork_device), and only a particle that the reset state holds has one: a particle added by
 *   sb_batch_add_particles_device since then has no reference until a checkpoint.  Right after a checkpoint or a reset, before any
 *   step, every reference equals the current position.
 * Matched members: a member of a group is FINITE when all six floats of its record are (position, velocity, acceleration: the
 *   rule of sb_batch_summary_device's word 4).  It is MATCHED when it is finite and has a reference whose two floats are finite.
 *   Everything below word 4 of a row counts all members; every sum is over the matched members alone.
 * Sums: eleven, in double, each pinned as sb_batch_summary_device pins its sums, restricted to the group's matched members: leaf i
 *   is the value at DATA index i if particle i is a matched member of the group, else +0.0; i = 0 .. W-1, W the smallest power of
 *   two >= max_particles; for h = W/2 .. 1: s[i] += s[i + h]; a sum that is zero is written as +0.0.  With every float cast to
 *   double first (so every product is exact and a leaf has one rounding) the leaves of a particle at (x, y) with velocity
 *   (vx, vy) and reference (X, Y) are
 *     x, y, X, Y, vx, vy,   D = x*X + y*Y,   C = X*y - Y*x,   Q = x*x + y*y,   Q0 = X*X + Y*Y,   L = x*vy - y*vx
 *   and their sums are written Sx, Sy, SX, SY, Svx, Svy, D, C, Q, Q0, L below.
 * Derived, in double, one rounding per operator, exactly these expressions, n the number of matched members as a double:
 *     a  = D  - (Sx*SX + Sy*SY) / n        b  = C - (SX*Sy - SY*Sx) / n
 *     I  = Q  - (Sx*Sx + Sy*Sy) / n        I0 = Q0 - (SX*SX + SY*SY) / n
 *     Lc = L  - (Sx*Svy - Sy*Svx) / n
 *   a and b are the dot and cross moments about the two centroids: the rotation that best carries the reference onto the current
 *   shape is atan2(b, a).  I and I0 are the moments of inertia (unit masses) of the current and the reference shape about their
 *   centroids, Lc the angular momentum about the current centroid.  The call takes no square root and no arc tangent.
 * moments[s][k] = {a, b, I, I0, Lc, n, 0, 0}.  With n == 0 -- the empty row included -- words 0 .. 4 are the quiet NaN
 *   0x7FF8000000000000, n and the padding 0.
 * rows[s][k], every float rounded once from its double:
 *    0  particles of the group (finite or not)       1  the label (<= 1023: exact as a float)
 *    2  matched members n                            3  members that are not matched (word 0 - word 2)
 *    4, 5  Sx / n, Sy / n: the current centroid      6, 7  SX / n, SY / n: the reference's centroid
 *    8, 9  Svx / n, Svy / n: the mean velocity      10, 11  a, b
 *   12, 13  I, I0                                   14  Lc
 *   15  Lc / I if I > 0, else NaN: the angular velocity
 *   16  I / I0 if I0 > 0, else NaN: the squared stretch
 *   17 .. 23  0
 *   With n == 0 words 4 .. 16 are the quiet NaN 0x7FC00000.  The EMPTY ROW: words 0, 2, 3 and 17 .. 23 are 0, word 1 is -1, words
 *   4 .. 16 NaN.  A scene never uploaded, and a scene without particles, give empty rows and rank -1.
 * Consequence: where every finite member of a group is matched, words 4, 5, 8, 9 equal words 6 .. 9 of the same row of
 * sb_batch_body_summary_device by their bits.
 * Errors: SB_ERR_INVALID for a NULL handle, NULL labels, rows, moments and rank all NULL, max_rows of 0 or above max_particles, a
 * pointer that is not 4-byte aligned, moments that is not 8-byte aligned -- before anything touches a device. */
#define SB_BATCH_POSE_WORDS 24u
#define SB_BATCH_POSE_MOMENT_WORDS 8u
sb_status sb_batch_pose_device(sb_batch *b,
        const void *device_labels_i32 /* [n_scenes][max_particles] int32, required */,
        const void *device_ref_f32    /* [n_scenes][max_particles][2] float {X, Y} at particle DATA indices, or NULL: the reset state */,
        uint32_t max_rows             /* 1 .. max_particles */,
        void *device_rows_f32         /* [n_scenes][max_rows][SB_BATCH_POSE_WORDS] float or NULL */,
        void *device_moments_f64      /* [n_scenes][max_rows][SB_BATCH_POSE_MOMENT_WORDS] double or NULL; 8-byte aligned */,
        void *device_rank_i32         /* [n_scenes][max_particles] int32 or NULL */);

/* ---- particle and wall contacts of every scene, reported on the device ----
 * sb_batch_contacts_device -- who touches whom, and who touches a wall, in ONE launch.
 * Particle set: the particles of a scene are its slots 0 .. metadata.particle_i_c - 1, named by their DATA index like the rows of
 *   sb_batch_read_state_device; their coordinates are the current particle records (what sb_batch_read_state_device would export
 *   at this point of the stream).
 * Particle contact: two distinct particles i and j TOUCH iff dist == 0 or dist < particle_radius * 2.0f, where dx = xj - xi,
 *   dy = yj - yi, dist = sqrt(dx * dx + dy * dy) in the library's arithmetic (binary32, one rounding per operator, correctly
 *   rounded sqrt): the expressions of the frame kernel's collision loop, so this is exactly the set of pairs the next substep's
 *   collision loop acts on (compute.wgsl:150-155).  The relation is symmetric.  A NaN or infinite dist is no contact.  The result
 *   does NOT depend on the batch's collision_mode: with SB_COLLIDE_OFF the same geometric set is reported.
 * Wall contact: lo = particle_radius, hi = bounds_size - particle_radius in float, as the step computes them; the bits are
 *   SB_BATCH_WALL_LEFT x <= lo, _RIGHT x >= hi, _LOW y <= lo, _HIGH y >= hi.  A particle the step has clamped sits exactly on lo or
 *   hi.  A NaN coordinate sets no bit.
 *   touch[s][i]   SB_BATCH_CONTACT_WORDS words per particle data index: 0 the number of particles touching i, 1 the number of those
 *                 whose label differs from i's (-1 when device_labels_i32 is NULL), 2 the wall bits, 3 the smallest data index of a
 *                 particle touching i (-1: none).  A row where no particle lives is {0, labels ? 0 : -1, 0, -1}.
 *   pairs[s]      one {i, j} per touching pair of the scene, i < j as data indices, in ascending lexicographic order of (i, j) (the
 *                 definition names no schedule); rows from the number of listed pairs up to max_pairs are {-1, -1}: every word is
 *                 written.  A scene of more than max_pairs pairs lists the first max_pairs in that order.  With
 *                 SB_BATCH_CONTACTS_OTHER_BODY only pairs whose labels differ are listed; order and truncation stay the same.
 *   counts[s]     SB_BATCH_CONTACT_WORDS words: 0 touching pairs (the true number, however small max_pairs is), 1 pairs whose labels
 *                 differ (-1 without labels), 2 particles with a nonzero wall word, 3 particles that touch at least one other.  A
 *                 scene with no particles, or one never uploaded, gives {0, 0 or -1, 0, 0}.
 * Labels ([n_scenes][max_particles] int32, as sb_batch_bodies_device writes them) are only compared for equality with each other
 * and never used as an index: stale or arbitrary labels cannot fault, they only mean what the caller made them mean.
 * Any of touch / pairs / counts may be NULL (not written), not all of them.  The call only ENQUEUES and only READS the batch:
 * frame, contacts, frame equals frame, frame bit for bit.
 * Errors: SB_ERR_INVALID for a NULL handle, an unknown flag bit, SB_BATCH_CONTACTS_OTHER_BODY without labels, touch, pairs and
 * counts all NULL, pairs non-NULL with max_pairs == 0, a pointer that is not 4-byte aligned -- before anything touches a device. */
#define SB_BATCH_CONTACT_WORDS 4u          /* words of a per-particle row and of a per-scene row */
#define SB_BATCH_CONTACTS_OTHER_BODY 1u    /* the pair list holds only pairs whose particles carry different labels */
#define SB_BATCH_WALL_LEFT 1u   /* x <= lo */
#define SB_BATCH_WALL_RIGHT 2u  /* x >= hi */
#define SB_BATCH_WALL_LOW 4u    /* y <= lo */
#define SB_BATCH_WALL_HIGH 8u   /* y >= hi */
sb_status sb_batch_contacts_device(sb_batch *b, uint32_t flags,
        const void *device_labels_i32 /* [n_scenes][max_particles] as sb_batch_bodies_device writes them, or NULL */,
        void *device_touch_i32        /* [n_scenes][max_particles][SB_BATCH_CONTACT_WORDS] or NULL */,
        void *device_pairs_i32        /* [n_scenes][max_pairs][2] or NULL */, uint32_t max_pairs,
        void *device_counts_i32       /* [n_scenes][SB_BATCH_CONTACT_WORDS] or NULL */);

/* ---- the beam graph of every scene: edge list, materials and a sorted adjacency on the device ----
 * sb_batch_graph_device -- which two particles every beam joins, with what material, and who hangs on whom, in ONE launch: the
 * beam half of a graph network's edge list (sb_batch_contacts_device's pair list is the contact half).
 *
 * DEFINITION.  The graph of a scene is defined on what sb_batch_load_scene would return at that point of the stream.
 * Nodes are the scene's particles, at particle DATA indices: the rows of sb_batch_read_state_device and of the contacts report.
 * Edges are its LISTED beams, at beam DATA indices.  A beam is LIVE by sb_batch_bodies_device's rule, word for word: a beam slot
 * < metadata.beam_i_c names its data index; a pending break flag still connects.  A live beam is LISTED unless
 * SB_GRAPH_SKIP_PENDING is set and its pending break flag is raised: with that flag the graph is what the next delete pass will
 * leave.  A listed beam d whose record's particle_pair is (a, b) -- low half, high half -- has two HALF-EDGES: side 0 at a with
 * neighbour b, side 1 at b with neighbour a.  The DEGREE of a particle is the number of half-edges at it (parallel beams count
 * each); a data index that holds no particle has degree 0.
 *
 * OUTPUTS.  Each may be NULL (not wanted); int32 unless said; every element of an output that is passed is written.
 *   ends[s][d]      {a, b}, particle data indices, at beam data index d; {-1, -1} where d is not a listed beam.  Row d lines up
 *                   with row d of sb_batch_read_state_device's beams: beam state becomes edge features by plain indexing.
 *   material[s][d]  float32 {length, spring, damp, yield_strain, strain_break_limit} of the beam's material row, verbatim bits;
 *                   zeros where d is not listed.  (After sb_batch_add_beams_device the caller holds no host copy of these.)
 *   row_ptr[s]      max_particles + 1 words: the exclusive prefix sum of the degrees over particle data indices;
 *                   row_ptr[s][max_particles] is the number of half-edges, twice the listed beams.
 *   nbr[s]          2 * max_beams rows {neighbour, beam data index}: the half-edges at particle p are rows row_ptr[p] ..
 *                   row_ptr[p + 1] - 1, in ascending order of beam data index (a beam from p to p: side 0, then side 1).  That order
 *                   is unique, so the array is the same bits on every run.  {-1, -1} behind the last half-edge.
 *   counts[s]       SB_BATCH_GRAPH_COUNT_WORDS words: 0 listed beams, 1 particles of degree >= 1, 2 the largest degree, 3 the
 *                   smallest data index of a particle of that degree (-1: no beam listed).
 * A scene never uploaded gives ends and nbr of -1, zero materials and row_ptr, counts {0, 0, 0, -1}.
 * It only ENQUEUES on the batch's stream and only READS the batch: frame, graph, frame equals frame, frame bit for bit.  Integers
 * only.  Errors, before anything touches a device: SB_ERR_INVALID for a NULL handle, unknown flag bits, a pointer that is not
 * 4-byte aligned, nbr without row_ptr.  With every output NULL the call is SB_OK and enqueues nothing.
 * sb_batch_get_info: "graph_count_words", "graph_material_words", "graph_lds_bytes" (LDS of one workgroup at this batch's
 * capacity), "graph_kernel_vgprs", "graph_kernel_scratch_bytes". */
/* flags: SB_GRAPH_SKIP_PENDING (above, with sb_graph_device) */
#define SB_BATCH_GRAPH_COUNT_WORDS 4u
#define SB_BATCH_GRAPH_MATERIAL_WORDS 5u
sb_status sb_batch_graph_device(sb_batch *b, uint32_t flags,
        void *device_ends_i32     /* [n_scenes][max_beams][2] or NULL */,
        void *device_material_f32 /* [n_scenes][max_beams][SB_BATCH_GRAPH_MATERIAL_WORDS] float or NULL */,
        void *device_row_ptr_i32  /* [n_scenes][max_particles + 1] or NULL */,
        void *device_nbr_i32      /* [n_scenes][2 * max_beams][2] or NULL; needs row_ptr */,
        void *device_counts_i32   /* [n_scenes][SB_BATCH_GRAPH_COUNT_WORDS] or NULL */);

/* ---- range sensors: ray casts per scene on the device, bit for bit ----
 * sb_batch_raycast_device -- "how far is the nearest thing in this direction, and what is it?": every scene gets its own k rays,
 * k <= SB_BATCH_RAY_MAX, in ONE launch; for every ray the answer is the nearest hit among the scene's particles (discs), its live
 * beams (segments) and the four walls.  device_rays is [n_scenes][k] sb_batch_ray.
 *
 * DEFINITION.  The arithmetic is the library's: binary32, one rounding per operator in the order written, correctly rounded / and
 * sqrt.  A comparison with a NaN is false.  Infinities follow the operators.
 * Ray row.  The ray is O + t D, O = (ox, oy), D = (dx, dy), for 0 <= t <= tmax.  D is not normalised: t is in units of |D| (pass a
 *   unit vector to get distances).  mask == 0 is an EMPTY row.  Otherwise the row is INVALID when an unknown mask bit is set; or
 *   ox, oy, dx or dy is not finite; or tmax is not >= 0 (a NaN fails; +inf is legal); or reserved != 0; or skip_label != -1 while
 *   device_labels_i32 is NULL.
 * Geometry: what sb_batch_load_scene would see at this point of the stream.
 *   Particles (SB_RAY_PARTICLES): the slots < metadata.particle_i_c at their current positions, named by DATA index; the radius is
 *     sb_batch_options.particle_radius, r2 = r * r computed once.
 *   Beams (SB_RAY_BEAMS): the live beam slots < metadata.beam_i_c, named by data index -- a pending break flag still counts, as for
 *     sb_batch_bodies_device --, each the segment between the current positions of its two endpoint particles; no thickness.
 *   Walls (SB_RAY_WALLS): the lines x = 0, x = bounds_size, y = 0, y = bounds_size.
 *   A scene never uploaded has no particles and no beams; its walls are still there.
 * Disc at (cx, cy).  wx = cx - ox, wy = cy - oy, a = dx*dx + dy*dy, b = wx*dx + wy*dy, c = (wx*wx + wy*wy) - r2.  c <= 0 (the
 *   origin is inside): t = 0.  Otherwise a hit only if b > 0 and q = b*b - a*c satisfies q >= 0; then t = (b - sqrt(q)) / a.  A
 *   zero D therefore hits only discs that contain O.
 * Segment A -> B.  ex = bx - ax, ey = by - ay, wx = ax - ox, wy = ay - oy, den = dx*ey - dy*ex, tn = wx*ey - wy*ex,
 *   un = wx*dy - wy*dx.  den == 0 (parallel or degenerate): no hit.  den < 0: negate all three.  A hit iff 0 <= un && un <= den &&
 *   0 <= tn; then t = tn / den.
 * Walls.  dx < 0: t = (0 - ox) / dx, SB_BATCH_WALL_LEFT; dx > 0: t = (bounds_size - ox) / dx, SB_BATCH_WALL_RIGHT; likewise in y
 *   with SB_BATCH_WALL_LOW and SB_BATCH_WALL_HIGH.  The other coordinate is not tested: from inside the box the nearest of the at
 *   most two candidates is the exit point; from outside the expressions still define the answer.
 * Every candidate.  t = t + 0.0f (so -0 becomes +0); it is kept iff t >= 0 && t <= tmax.
 * Skipping.  A particle whose label equals the row's skip_label is ignored, and so is a beam whose endpoint A (the low half of its
 *   record's particle_pair) carries that label; -1 ignores nothing.  Labels are [n_scenes][max_particles] int32 at particle data
 *   indices, as sb_batch_bodies_device writes them; they are only compared and never used as an index, so stale or arbitrary
 *   labels cannot fault.  A sensor that rides on a body sees past its own body this way.
 * Winner.  The smallest (t, kind, index): t by its bit pattern (non-negative, so the bits order as the floats do); kind particle 1
 *   < beam 2 < wall 3; index the particle data index, the beam data index or the wall word.  It is the minimum of the 64-bit keys
 *   (bits(t) << 32) | (kind << 16) | index: an integer minimum, the same bits whatever the schedule.
 *
 * OUTPUTS.  Each may be NULL, not all of them; every word of an output that is passed is written.
 *   t[s][j]       float32: the hit's t; on a miss the row's tmax bits, verbatim; 0 for an empty or invalid row.
 *   hit[s][j]     SB_BATCH_RAY_HIT_WORDS int32 {kind, index, label}.  kind: 0 miss, 1 particle, 2 beam, 3 wall, -1 empty row, -2
 *                 invalid row.  index: -1 where there is no hit.  label: the label of the hit particle, or of the hit beam's
 *                 endpoint A; -1 for walls, for misses and without labels.
 *   counts[s]     SB_BATCH_RAY_COUNT_WORDS int32: 0 valid rows (neither empty nor invalid), 1 hits on particles, 2 hits on beams,
 *                 3 hits on walls.
 * It only ENQUEUES on the batch's stream and only READS the batch: frame, raycast, frame equals frame, frame bit for bit.
 * Errors, before anything touches a device: SB_ERR_INVALID for a NULL handle, an unknown flag bit (no flag is defined yet: flags
 * must be 0), k > SB_BATCH_RAY_MAX, NULL rows with k > 0, all outputs NULL, a pointer that is not 4-byte aligned.  k == 0 is SB_OK
 * and enqueues nothing.  sb_batch_get_info: "ray_max", "ray_hit_words", "ray_count_words", "raycast_lds_bytes" (LDS of one
 * workgroup at this batch's capacity), "raycast_kernel_vgprs", "raycast_kernel_scratch_bytes". */
typedef struct sb_batch_ray { /* 32 bytes */
    uint32_t mask;           /* SB_RAY_*; 0: empty row */
    float ox, oy, dx, dy;    /* origin and direction */
    float tmax;              /* >= 0; +inf: no limit */
    int32_t skip_label;      /* -1: nothing is skipped */
    uint32_t reserved;       /* 0 */
} sb_batch_ray;
#define SB_BATCH_RAY_MAX 256u           /* rows per scene and call */
#define SB_RAY_PARTICLES 1u
#define SB_RAY_BEAMS 2u
#define SB_RAY_WALLS 4u
#define SB_BATCH_RAY_HIT_WORDS 3u
#define SB_BATCH_RAY_COUNT_WORDS 4u
#define SB_BATCH_RAY_MISS 0             /* hit[0] */
#define SB_BATCH_RAY_PARTICLE 1
#define SB_BATCH_RAY_BEAM 2
#define SB_BATCH_RAY_WALL 3
#define SB_BATCH_RAY_EMPTY (-1)
#define SB_BATCH_RAY_INVALID (-2)
sb_status sb_batch_raycast_device(sb_batch *b, uint32_t flags,
        const void *device_rays       /* [n_scenes][k] sb_batch_ray */, uint32_t k,
        const void *device_labels_i32 /* [n_scenes][max_particles] as sb_batch_bodies_device writes them, or NULL */,
        void *device_t_f32            /* [n_scenes][k] float or NULL */,
        void *device_hit_i32          /* [n_scenes][k][SB_BATCH_RAY_HIT_WORDS] or NULL */,
        void *device_counts_i32       /* [n_scenes][SB_BATCH_RAY_COUNT_WORDS] or NULL */);

/* ---- proximity queries: nearest particle, beam or wall per point on the device, bit for bit ----
 * sb_batch_nearest_device -- "what is nearest to this point, how far is it, and how much is within reach?": every scene gets its own
 * k points, k <= SB_BATCH_NEAR_MAX, in ONE launch; for every point the answer is the nearest among the scene's particles (their
 * centres), its live beams (segments) and the four walls, the closest point on it, and how many particles and beams lie within
 * rmax.  device_points is [n_scenes][k] sb_batch_near_point.
 *
 * DEFINITION.  The arithmetic is the library's: binary32, one rounding per operator in the order written, correctly rounded / and
 * sqrt.  A comparison with a NaN is false.  Infinities follow the operators.
 * Row.  The query point is (px, py), the reach rmax; rmax2 = rmax * rmax, computed once.  mask == 0 is an EMPTY row.  Otherwise the
 *   row is INVALID when an unknown mask bit is set; or px or py is not finite; or rmax is not >= 0 (a NaN fails; +inf is legal); or
 *   a reserved word is not 0; or skip_label != -1 while device_labels_i32 is NULL.
 * Geometry: sb_batch_raycast_device's, what sb_batch_load_scene would see at this point of the stream.
 *   Particles (SB_NEAR_PARTICLES): the slots < metadata.particle_i_c at their current positions, named by DATA index.
 *   Beams (SB_NEAR_BEAMS): the live beam slots < metadata.beam_i_c, named by data index -- a pending break flag still counts --, each
 *     the segment between the current positions of its two endpoint particles; no thickness.
 *   Walls (SB_NEAR_WALLS): the lines x = 0, x = bounds_size, y = 0, y = bounds_size.
 *   A scene never uploaded has no particles and no beams; its walls are still there.
 * Every primitive has a closest point Q and the squared distance d2 to it.
 * Particle at C = (cx, cy).  Q = C (centres, as an editor's hover test measures, not disc surfaces): vx = cx - px, vy = cy - py,
 *   d2 = vx*vx + vy*vy.
 * Segment A -> B.  ex = bx - ax, ey = by - ay, wx = px - ax, wy = py - ay, ee = ex*ex + ey*ey, we = wx*ex + wy*ey.  If !(we > 0):
 *   Q = A (a degenerate beam has ee = 0, so we = 0: it answers as its endpoint A and nothing is divided).  Else if !(we < ee): Q = B.
 *   Else u = we / ee and Q = (ax + u*ex, ay + u*ey).  Then vx = qx - px, vy = qy - py, d2 = vx*vx + vy*vy: at a clamped end this is
 *   the particle's expression on that endpoint, bit for bit.
 * Walls.  Left: vx = 0 - px, d2 = vx*vx, Q = (0, py), index SB_BATCH_WALL_LEFT.  Right: vx = bounds_size - px, Q = (bounds_size, py),
 *   SB_BATCH_WALL_RIGHT.  Low: vy = 0 - py, d2 = vy*vy, Q = (px, 0), SB_BATCH_WALL_LOW.  High: vy = bounds_size - py,
 *   Q = (px, bounds_size), SB_BATCH_WALL_HIGH.
 * Kept.  A primitive is kept iff d2 <= rmax2.  A NaN d2 (a NaN coordinate) is never kept.  A d2 of +inf (an infinite coordinate, or
 *   an overflow) is kept only when rmax2 is +inf too, that is under rmax = +inf or an rmax whose square overflows: the operators
 *   decide, nothing is special-cased.
 * Skipping.  The ray cast's rule: a particle whose label equals the row's skip_label is ignored, and so is a beam whose endpoint A
 *   (the low half of its record's particle_pair) carries that label; -1 ignores nothing.  Labels are [n_scenes][max_particles]
 *   int32 at particle data indices; they are only compared and never used as an index, so stale or arbitrary labels cannot fault.
 * Winner.  Among the kept, the smallest (d2, kind, index): the minimum of the 64-bit keys (bits(d2) << 32) | (kind << 16) | index,
 *   kind particle 1 < beam 2 < wall 3, index the particle data index, the beam data index or the wall word.  d2 is a sum of squares
 *   and never -0, so its bits order as the floats do.  A particle therefore beats the beams that end in it, and between equals the
 *   smaller data index wins.  It is an integer minimum: the same bits whatever the schedule.
 *
 * OUTPUTS.  Each may be NULL, not all of them; every word of an output that is passed is written.
 *   d[s][j]       float32: sqrt(d2) of the winner; on a miss (nothing kept) the row's rmax bits, verbatim; 0 for an empty or invalid
 *                 row.
 *   hit[s][j]     SB_BATCH_NEAR_HIT_WORDS int32 {kind, index, label}, the ray cast's: kind 0 miss, 1 particle, 2 beam, 3 wall, -1
 *                 empty row, -2 invalid row; index -1 where there is no winner; label the label of the winning particle, or of the
 *                 winning beam's endpoint A; -1 for walls, for misses and without labels.
 *   point[s][j]   2 float32: the winner's closest point Q, computed again from the winner by the expressions above -- where a grab
 *                 attaches.  On a miss the query point's bits; 0, 0 for an empty or invalid row.
 *   within[s][j]  2 int32: how many particles that are not skipped, and how many live beams that are not skipped, were kept
 *                 (d2 <= rmax2).  A class whose mask bit is off gives 0; an empty or invalid row gives 0, 0.  Walls are not counted.
 *   counts[s]     SB_BATCH_NEAR_COUNT_WORDS int32: 0 valid rows (neither empty nor invalid), 1 rows whose nearest is a particle, 2 a
 *                 beam, 3 a wall.
 * It only ENQUEUES on the batch's stream and only READS the batch: frame, nearest, frame equals frame, frame bit for bit.
 * Errors, before anything touches a device: SB_ERR_INVALID for a NULL handle, an unknown flag bit (no flag is defined yet: flags
 * must be 0), k > SB_BATCH_NEAR_MAX, NULL rows with k > 0, all outputs NULL, a pointer that is not 4-byte aligned.  k == 0 is SB_OK
 * and enqueues nothing.  sb_batch_get_info: "near_max", "near_hit_words", "near_count_words", "nearest_lds_bytes" (LDS of one
 * workgroup at this batch's capacity), "nearest_kernel_vgprs", "nearest_kernel_scratch_bytes". */
typedef struct sb_batch_near_point { /* 32 bytes */
    uint32_t mask;           /* SB_NEAR_*; 0: empty row */
    float px, py;            /* the query point */
    float rmax;              /* >= 0; +inf: no limit */
    int32_t skip_label;      /* -1: nothing is skipped */
    uint32_t reserved[3];    /* 0 */
} sb_batch_near_point;
#define SB_BATCH_NEAR_MAX 256u          /* rows per scene and call */
#define SB_NEAR_PARTICLES 1u
#define SB_NEAR_BEAMS 2u
#define SB_NEAR_WALLS 4u
#define SB_BATCH_NEAR_HIT_WORDS 3u
#define SB_BATCH_NEAR_COUNT_WORDS 4u
#define SB_BATCH_NEAR_MISS 0            /* hit[0] */
#define SB_BATCH_NEAR_PARTICLE 1
#define SB_BATCH_NEAR_BEAM 2
#define SB_BATCH_NEAR_WALL 3
#define SB_BATCH_NEAR_EMPTY (-1)
#define SB_BATCH_NEAR_INVALID (-2)
sb_status sb_batch_nearest_device(sb_batch *b, uint32_t flags,
        const void *device_points     /* [n_scenes][k] sb_batch_near_point */, uint32_t k,
        const void *device_labels_i32 /* [n_scenes][max_particles] as sb_batch_bodies_device writes them, or NULL */,
        void *device_d_f32            /* [n_scenes][k] float or NULL */,
        void *device_hit_i32          /* [n_scenes][k][SB_BATCH_NEAR_HIT_WORDS] or NULL */,
        void *device_point_f32        /* [n_scenes][k][2] float or NULL */,
        void *device_within_i32       /* [n_scenes][k][2] or NULL */,
        void *device_counts_i32       /* [n_scenes][SB_BATCH_NEAR_COUNT_WORDS] or NULL */);

/* ---- beam and contact forces per particle of every scene, reported on the device, bit for bit ----
 * sb_batch_forces_device -- how hard does every beam pull and every contact push?  For every scene, in ONE launch that only reads
 * the batch and only enqueues, the forces the NEXT substep would compute from the CURRENT state.  Nothing is applied: no yield, no
 * last_length update, no break flag, no particle moved.
 *
 * Let P be the scene's particle slots and Bc its live beam slots (metadata.particle_i_c / beam_i_c, clamped to the capacity; 0 in
 * a scene never uploaded).  All float expressions are the step's: binary32, one rounding per operator (no contraction), IEEE sqrt
 * and divide.
 *
 * Beam part.  It covers every beam slot j < Bc: exactly the set the frame kernel's beam phase evaluates.  A pending break flag
 *   still counts.  A beam removed by a delete pass does not.  Each beam is evaluated as the step evaluates it (compute.wgsl:103-130)
 *   from the current positions of its endpoints, its current {target_length, last_length} and its material row: diff = pb - pa,
 *   len = length(diff) -- a beam of length zero takes diff = (0, -1e-10) and its length, the guard of :104-107 --
 *   force_mag = (target_length - len) * spring + (last_length - len) * damp, n = diff * (1 / len), f = force_mag * n, and the four
 *   i32 contributions ax = i32(-(f.x * 65536)), ay = i32(-(f.y * 65536)), bx = i32(f.x * 65536), by = i32(f.y * 65536).  The
 *   conversion is v_cvt_i32_f32's: truncate toward zero, saturate at INT_MIN / INT_MAX, NaN -> 0.
 *   Per particle these contributions are summed with wrapping 32-bit adds: beam_i32[s][i] = {sum x, sum y} at particle DATA index
 *   i, the words the particle's integration would receive as fx, fy.  Being integers, they do not depend on summation order.
 *   tension[s][d], float at beam DATA index d, is the beam's force_mag; 0 where no evaluated beam lives.  It is signed, with the
 *   reference's sign: positive where the beam is shorter than its target and pushes its endpoints apart, negative where it is
 *   stretched and pulls them together.
 * Contact part.  For particle slot s, take the partners o != s in ASCENDING SLOT ORDER.  A partner satisfies dist == 0 ||
 *   dist < 2r, with dx = xo - xs, dy = yo - ys, dist = sqrt(dx * dx + dy * dy), 2r = particle_radius * 2.0f: the contact test of
 *   sb_batch_contacts_device; the batch's collision_mode does not matter.  Both sums start at +0 and accumulate exactly the terms
 *   the step's collision loop (compute.wgsl:156-168) would subtract from the particle's acceleration and velocity:
 *     push    -= (n * overlap * 0.5) * inv_dt2     n = (dx, dy) * (1 / dist), overlap = 2r - dist; where dt^2 = time_step^2 is no
 *                                                  power of two the product with inv_dt2 is the division by dt^2
 *     impulse -= impulse_normal * n + impulse_tangent * t
 *                                                  t = (-n.y, n.x), u = v_s - v_o, impulse_normal = elasticity_coeff * dot(u, n),
 *                                                  elasticity_coeff = (elasticity + 1) / 2, max_friction = impulse_normal *
 *                                                  friction, impulse_tangent = clamp(dot(u, t), -max_friction, max_friction)
 *   with the scene's current physics constants.  A dist == 0 partner counts as a partner with depth 2r and adds nothing to push
 *   or impulse (the step only shifts p.y there).  depth is the largest 2r - dist over the partners, 0 with no partner.
 *   With SB_BATCH_FORCES_OTHER_BODY and a labels tensor only partners whose label differs from s's are taken (labels: [n_scenes]
 *   [max_particles] int32 at particle data indices, as sb_batch_bodies_device writes them; only compared with each other, never
 *   used as an index).  Without the flag the labels are not looked at.
 *   rows[s][i]    SB_BATCH_FORCE_WORDS floats at particle DATA index i: 0, 1 beam_x, beam_y = (float)beam_i32 * 2^-16 (the exact
 *                 product of the particle's integration); 2, 3 push_x, push_y; 4, 5 impulse_x, impulse_y; 6 depth; 7 partners,
 *                 the number of partners taken as an exact float.  A row where no particle lives is eight +0 words: data indices
 *                 that hold no particle, scenes never uploaded, empty scenes.  (beam_i32 is {0, 0} there.)
 *   counts[s]     SB_BATCH_FORCE_COUNT_WORDS int32: 0 particles P, 1 beam slots evaluated (Bc; 0 where P is 0), 2 particles with
 *                 at least one partner taken, 3 beams whose force_mag is not finite.
 * Every word of every output that is passed is written; any of them may be NULL (all of them: SB_OK, nothing is enqueued).  The
 * call only ENQUEUES on the batch's stream and only READS the batch: frame, forces, frame equals frame, frame bit for bit; two
 * calls give the same bits.
 * Errors, before anything touches a device: SB_ERR_INVALID for a NULL handle, an unknown flag bit, SB_BATCH_FORCES_OTHER_BODY
 * without labels, a pointer that is not 4-byte aligned.  sb_batch_get_info: "force_words", "force_count_words",
 * "forces_kernel_vgprs", "forces_kernel_scratch_bytes", "forces_lds_bytes" (LDS of one workgroup at this batch's capacity),
 * "forces_cells_per_side" (G of the G x G cells scenes of at least "grid_min_particles" particles are binned into; 0: none). */
#define SB_BATCH_FORCE_WORDS 8u            /* floats of a per-particle row */
#define SB_BATCH_FORCE_COUNT_WORDS 4u      /* words of a per-scene row */
#define SB_BATCH_FORCES_OTHER_BODY 1u      /* only partners whose label differs from the particle's are taken */
sb_status sb_batch_forces_device(sb_batch *b, uint32_t flags,
        const void *device_labels_i32 /* [n_scenes][max_particles] as sb_batch_bodies_device writes them, or NULL */,
        void *device_rows_f32         /* [n_scenes][max_particles][SB_BATCH_FORCE_WORDS] float or NULL */,
        void *device_beam_i32         /* [n_scenes][max_particles][2] or NULL */,
        void *device_tension_f32      /* [n_scenes][max_beams] float or NULL */,
        void *device_counts_i32       /* [n_scenes][SB_BATCH_FORCE_COUNT_WORDS] or NULL */);

/* ---- range sensors over the whole scene of ONE engine: ray casts on the device, bit for bit ----
 * sb_raycast_device / sb_raycast -- sb_batch_raycast_device's question asked of an sb_engine: n_rays rows of sb_batch_ray (the same
 * 32 bytes, masks and verdicts), for each the nearest hit among the scene's particles, live beams and walls.  The DEFINITION is the
 * one above, word for word: the disc, segment and wall tests, t + 0.0f, 0 <= t <= tmax, skipping by the label of the particle or of
 * the beam's endpoint A, the winner the smallest (t bits, kind, index).  The geometry is what sb_load_buffers would return at this
 * point of the stream: particles at DATA indices at their current positions; beams LIVE by sb_bodies' rule (a caller slot of the
 * latest upload that neither a delete pass nor a plan-keeping upload has removed; a pending break flag still counts), named by beam
 * data index; radius and bounds are sb_options'.  A scene that fits a batch gives exactly the batch's t and hit rows.
 * The key is wider: (bits(t) << 32) | (kind << 30) | index -- the same order, so the same winners, with room for the indices of an
 * engine; max_particles or max_beams above 2^30: SB_ERR_UNSUPPORTED.
 *   labels   int32 [max_particles] at particle data indices (sb_bodies' labels, or the caller's own), or NULL; only compared.
 *   t        float32 [n_rays]: the hit's t; the row's tmax bits on a miss; 0 for an empty or invalid row.
 *   hit      int32 [n_rays][SB_BATCH_RAY_HIT_WORDS] {kind, index, label} as above.
 *   counts   int64 [SB_RAYCAST_COUNT_WORDS]: 0 valid rows, 1 hits on particles, 2 on beams, 3 on walls; then three COST words,
 *            pure functions of the rows' bits, the positions and the cells: 4 rows answered by the sweep, 5 particles outside the
 *            grid, 6 long beams; 7 is 0.
 * Each output may be NULL, not all of them; every word of one that is passed is written.
 * COST.  The primitives are sorted into G x G cells over [0, bounds]^2, cell = max(2 r (1 + 1/64), bounds / G): by default the
 * largest G with G * G <= particles / 2 (at least 1, at most 8192) that keeps the cell that wide; cells_per_side != 0 replaces
 * particles / 2's G as the cap (one cell where the radius or the bounds lie outside [2^-20, 2^30]).  A particle is IN-GRID iff both
 * coordinates are finite and in [0, bounds]; a live beam is SHORT iff both endpoints are in-grid and their cells (x / cell, y / cell in
 * float32, truncated, at most G - 1) differ by at most one per axis.  A row is WALKABLE iff ox and oy lie in [-bounds, 2 bounds] and
 * a = dx*dx + dy*dy (float32) lies in [2^-40, 2^40]; it looks only into the cells along its line (csrc/sb_ray_walk.h derives which
 * ones from the rounding of the tests; a row with SB_RAY_BEAMS walks the whole line, a row without stops once nothing further on
 * can win; a row with neither walks nothing).  So a row with SB_RAY_BEAMS -- mask 7 among them -- costs O(G) columns of a few cells
 * each whatever its tmax: a sensor that only needs particles and walls should say so in its mask.  Word 4 counts the valid rows that are not walkable: each is tested against every primitive.  Word 5 counts the
 * particles that are not in-grid, word 6 the live beams that are not short: EVERY valid row is tested against each of them, so a
 * scene full of them stays correct and gets slow.  The outputs never depend on G.
 * sb_raycast_device only ENQUEUES on the engine's stream, reads nothing back and waits for nothing but the one table build after
 * an upload (the shared scene tables, sb_cut_device's rows); it only READS the engine: frame, raycast, frame equals frame, frame
 * bit for bit.  sb_raycast is the host-copy convenience: rows and labels from host memory, the same launches, the outputs copied
 * back; it waits.
 * Errors, before anything touches a device: SB_ERR_INVALID for a NULL handle, a struct_size that is neither 0 nor the struct's, an
 * unknown flag (none is defined: flags must be 0), a nonzero reserved word, NULL rows with n_rays > 0, all outputs NULL, rows /
 * labels / t / hit not 4-byte or counts not 8-byte aligned, n_rays above 2^24, cells_per_side above 8192; SB_ERR_STATE before an
 * upload; SB_ERR_UNSUPPORTED with ranks or ghost zones, or capacities above 2^30.  n_rays == 0 is SB_OK and enqueues nothing.
 * sb_get_info: "raycast_cells_per_side" (the default rule on the scene as it is), "raycast_kernel_vgprs",
 * "raycast_kernel_scratch_bytes", "raycast_table_build_us". */
#define SB_RAYCAST_COUNT_WORDS 8u
typedef struct sb_raycast_options {
    uint32_t struct_size;    /* = sizeof(sb_raycast_options); 0 or a NULL pointer = all defaults */
    uint32_t flags;          /* none defined: 0 */
    uint32_t cells_per_side; /* 0: the default rule */
    uint32_t reserved[5];    /* zero */
} sb_raycast_options;
sb_status sb_raycast_device(sb_engine *e, const sb_raycast_options *opts, const void *device_rays /* [n_rays] sb_batch_ray */, uint32_t n_rays,
                            const void *device_labels_i32 /* [max_particles] or NULL */, void *device_t_f32 /* [n_rays] or NULL */,
                            void *device_hit_i32 /* [n_rays][SB_BATCH_RAY_HIT_WORDS] or NULL */,
                            void *device_counts_i64 /* [SB_RAYCAST_COUNT_WORDS] or NULL */);
sb_status sb_raycast(sb_engine *e, const sb_raycast_options *opts, const sb_batch_ray *rays, uint32_t n_rays, const int32_t *labels, float *t,
                     int32_t *hit, int64_t *counts);

/* ---- proximity queries over the whole scene of ONE engine, on the device, bit for bit ----
 * sb_nearest_device / sb_nearest -- sb_batch_nearest_device's question asked of an sb_engine: n_points rows of sb_batch_near_point
 * (the same 32 bytes, masks and verdicts), for each the nearest among the scene's particles (centres), live beams (segments) and the
 * four walls, the closest point on it, and how many particles and beams lie within rmax.  The DEFINITION is the one above, word for
 * word: particle centres, the clamped projection on a beam, the walls; rmax2 = rmax * rmax computed once, kept iff d2 <= rmax2;
 * skipping by the label of the particle or of the beam's endpoint A; the winner the smallest (d2 bits, kind, index).  The geometry is
 * sb_raycast_device's: what sb_load_buffers would return at this point of the stream, beams LIVE by sb_bodies' rule (a pending break
 * flag still counts), radius and bounds sb_options'.  A scene that fits a batch gives exactly the batch's d, hit, point and within
 * rows.  The key is the wide one, (bits(d2) << 32) | (kind << 30) | index: the same order, room for an engine's indices;
 * max_particles or max_beams above 2^30: SB_ERR_UNSUPPORTED.
 *   labels   int32 [max_particles] at particle data indices (sb_bodies' labels, or the caller's own), or NULL; only compared.
 *   d        float32 [n_points]: sqrt(d2) of the winner; the row's rmax bits on a miss; 0 for an empty or invalid row.
 *   hit      int32 [n_points][SB_BATCH_NEAR_HIT_WORDS] {kind, index, label} as above.
 *   point    float32 [n_points][2]: the winner's closest point, computed again from the winner by the definition's expressions; the
 *            query point's bits on a miss; 0, 0 for an empty or invalid row.
 *   within   int32 [n_points][2]: particles and beams kept, not skipped, mask bit on; 0, 0 for an empty or invalid row.
 *   counts   int64 [SB_NEAREST_COUNT_WORDS]: 0 valid rows, 1 winners that are particles, 2 beams, 3 walls; then three COST words,
 *            pure functions of the rows' bits, the positions, the cells and max_rings: 4 rows answered by the sweep, 5 particles
 *            outside the grid, 6 long beams; 7 is 0.
 * Each output may be NULL, not all of them; every word of one that is passed is written.
 * COST.  The grid is the ray casts': the same cells, the same sort, the same cells_per_side rule and cap.  A row is LOCAL iff px and py
 * lie in [-bounds, 2 bounds].  A local row looks into the cells round its point ring by ring (csrc/sb_near_walk.h derives which, and
 * when it may stop, from the rounding of the distances): it stops once nothing further on can be kept (rmax), or -- where within is
 * NULL -- once nothing further on can win.  A row whose walk has not stopped after max_rings rings (0: the default,
 * "nearest_max_rings"; rings that lie wholly outside the grid are not counted), and every row that is not local, is tested against
 * every primitive by the sweep: word 4.  So rmax = +inf with within costs a pass over the scene per row unless the rings cover the
 * grid -- the count of everything is a sum over everything; rmax = +inf without within stops at the winner.  Words 5 and 6 are the
 * ray casts': every row is tested against those leftovers.  The outputs never depend on cells_per_side or max_rings.
 * sb_nearest_device only ENQUEUES on the engine's stream, reads nothing back and waits for nothing but the one table build after an
 * upload; it only READS the engine: frame, nearest, frame equals frame, frame bit for bit.  sb_nearest is the host-copy convenience:
 * rows and labels from host memory, the same launches, the outputs copied back; it waits.
 * Errors, before anything touches a device: SB_ERR_INVALID for a NULL handle, a struct_size that is neither 0 nor the struct's, an
 * unknown flag (none is defined: flags must be 0), a nonzero reserved word, NULL rows with n_points > 0, all outputs NULL, rows /
 * labels / d / hit / point / within not 4-byte or counts not 8-byte aligned, n_points above 2^24, cells_per_side or max_rings above
 * 8192; SB_ERR_STATE before an upload; SB_ERR_UNSUPPORTED with ranks or ghost zones, or capacities above 2^30.  n_points == 0 is SB_OK
 * and enqueues nothing.  sb_get_info: "nearest_cells_per_side" (the default rule on the scene as it is), "nearest_max_rings" (the
 * default), "nearest_kernel_vgprs", "nearest_kernel_scratch_bytes". */
#define SB_NEAREST_COUNT_WORDS 8u
typedef struct sb_nearest_options {
    uint32_t struct_size;    /* = sizeof(sb_nearest_options); 0 or a NULL pointer = all defaults */
    uint32_t flags;          /* none defined: 0 */
    uint32_t cells_per_side; /* 0: the default rule (sb_raycast_options') */
    uint32_t max_rings;      /* 0: the default; at most 8192 */
    uint32_t reserved[4];    /* zero */
} sb_nearest_options;
sb_status sb_nearest_device(sb_engine *e, const sb_nearest_options *opts, const void *device_points /* [n_points] sb_batch_near_point */,
                            uint32_t n_points, const void *device_labels_i32 /* [max_particles] or NULL */,
                            void *device_d_f32 /* [n_points] or NULL */, void *device_hit_i32 /* [n_points][SB_BATCH_NEAR_HIT_WORDS] or NULL */,
                            void *device_point_f32 /* [n_points][2] or NULL */, void *device_within_i32 /* [n_points][2] or NULL */,
                            void *device_counts_i64 /* [SB_NEAREST_COUNT_WORDS] or NULL */);
sb_status sb_nearest(sb_engine *e, const sb_nearest_options *opts, const sb_batch_near_point *points, uint32_t n_points, const int32_t *labels,
                     float *d, int32_t *hit, float *point, int32_t *within, int64_t *counts);

/* ---- beam and contact forces of the whole scene of ONE engine, on the device, bit for bit ----
 * sb_forces_device / sb_forces -- sb_batch_forces_device's question asked of an sb_engine: the forces the NEXT substep would compute
 * from the CURRENT state, in the step's own float arithmetic (binary32, one rounding per operator, IEEE sqrt and divide), with nothing
 * applied: no yield, no last_length update, no break flag, no particle moved.  The DEFINITION is the one above, word for word, for
 * the one scene; what an engine adds is said here.
 * Beam part.  It covers every caller beam slot of the latest upload that no delete pass has removed.  A pending break flag still
 *   counts.  A beam removed by a delete pass or by a plan-keeping upload does not.  Each beam is evaluated as the step evaluates it
 *   (compute.wgsl:103-130; sb_beam_eval) from the current positions of its endpoints, its current {target_length, last_length} --
 *   the floats sb_read_state_device exports at this point of the stream -- and its {spring, damp} as uploaded.  tension[d], float at
 *   beam DATA index d, is the beam's force_mag = (target_length - len) * spring + (last_length - len) * damp (the reference's sign:
 *   positive pushes the endpoints apart); 0 where no evaluated beam lives, up to max_beams.  The four i32 contributions
 *   (v_cvt_i32_f32: truncate, saturate, NaN -> 0) are summed per particle DATA index with wrapping 32-bit adds: beam_i32[i] =
 *   {sum x, sum y}; {0, 0} where no particle lives, up to max_particles.  Integers: no summation order.
 * Contact part.  For each particle, its partners (dist == 0 || dist < 2r: sb_contacts_device's test, whatever collision_mode is) are
 *   taken in ASCENDING MAPPING-SLOT ORDER, the order of the step's collision loop, and summed from +0 by the batch's expressions
 *   with the engine's current constants: friction, elasticity_coeff = (elasticity + 1) / 2 (sb_set_physics_constants or the
 *   upload's metadata, as the next substep would take them), and inv_dt2 / dt^2 of sb_options.subticks (the product where dt^2 is a
 *   power of two, the division where it is not).  With SB_FORCES_OTHER_BODY and labels only partners whose label differs from the
 *   particle's are taken (labels: int32 [max_particles] at particle data indices, sb_bodies_device's or the caller's own; only
 *   compared).  Without the flag the labels are not looked at.
 *   rows[i]   SB_FORCE_WORDS floats at particle DATA index i, the batch's columns: 0, 1 beam_x, beam_y = (float)beam_i32 * 2^-16;
 *             2, 3 push_x, push_y; 4, 5 impulse_x, impulse_y; 6 depth; 7 partners.  Eight +0 words where no particle lives, up to
 *             max_particles.
 *   counts    SB_FORCE_COUNT_WORDS int64: 0 particles, 1 beams evaluated, 2 particles with at least one partner taken, 3 beams
 *             whose force_mag is not finite.
 * A scene that fits a batch gives exactly the batch's rows, beam_i32 and tension for that scene.  With gravity 0, drag 0 and everything
 * at rest, forces then one substep: v == (push + beam) * time_step and stress == tension / 20, bit for bit.
 * Each output may be NULL, not all of them; every word of one that is passed is written.
 * sb_forces_device only ENQUEUES on the engine's stream -- two clears, a launch over the beams, sb_contacts_device's counting sort by
 * cell with records keyed by mapping slot, a launch over the sorted records, the rows where nobody lives, the counts -- reads nothing
 * back, no workgroup waits for another, and it waits for nothing but the one table build after an upload (the shared scene tables
 * with two more planes: mapping slot -> particle, {spring, damp} per beam slot; sb_cut_device's rows).  It only READS the engine:
 * frame, forces, frame equals frame, frame bit for bit; two calls give the same bits.  It works on every path, layout and collision
 * mode.  sb_forces is the host-copy convenience: labels from host memory, the same launches, the outputs copied back; it waits.
 * Errors, before anything touches a device: SB_ERR_INVALID for a NULL handle, a struct_size that is neither 0 nor the struct's, an
 * unknown flag bit, a nonzero reserved word, SB_FORCES_OTHER_BODY without labels, all outputs NULL, labels / rows / beam_i32 / tension
 * not 4-byte or counts not 8-byte aligned; SB_ERR_STATE before an upload; SB_ERR_UNSUPPORTED on an engine with ghost zones or peers
 * configured, and where the cell side is no ordinary number in a scene of more than 4096 particles (sb_contacts_device's rule; at or
 * below 4096 every pair is tested).  sb_get_info: "forces_cells_per_side" (of the scene as it is; 1: all pairs),
 * "forces_table_build_us" (host time of the last build of the tables the latest call read), "forces_kernel_vgprs",
 * "forces_kernel_scratch_bytes". */
#define SB_FORCE_WORDS 8u              /* floats of a per-particle row (SB_BATCH_FORCE_WORDS) */
#define SB_FORCE_COUNT_WORDS 4u        /* int64 words of counts */
#define SB_FORCES_OTHER_BODY 1u        /* only partners whose label differs from the particle's are taken */
typedef struct sb_forces_options {
    uint32_t struct_size;    /* = sizeof(sb_forces_options); 0 or a NULL pointer = all defaults: no flags */
    uint32_t flags;          /* SB_FORCES_OTHER_BODY */
    uint32_t reserved[6];    /* zero */
} sb_forces_options;
sb_status sb_forces_device(sb_engine *e, const sb_forces_options *opts, const void *device_labels_i32 /* [max_particles] or NULL */,
                           void *device_rows_f32 /* [max_particles][SB_FORCE_WORDS] float or NULL */,
                           void *device_beam_i32 /* [max_particles][2] or NULL */, void *device_tension_f32 /* [max_beams] float or NULL */,
                           void *device_counts_i64 /* [SB_FORCE_COUNT_WORDS] or NULL */);
sb_status sb_forces(sb_engine *e, const sb_forces_options *opts, const int32_t *labels, float *rows, int32_t *beam_i32, float *tension,
                    int64_t *counts);

/* scene i back into host buffers exactly as sb_load_buffers returns a single engine in the same state (counts in the metadata,
 * the mapping after the delete passes' stable in-place compactions, beam records with strain / stress; only records reachable
 * through the uploaded mapping are written; any pointer may be NULL).  SB_ERR_STATE for a scene never uploaded. */
sb_status sb_batch_load_scene(sb_batch *b, uint32_t scene, void *metadata, size_t metadata_bytes, void *mapping, size_t mapping_bytes,
                              void *particles, size_t particles_bytes, void *beams, size_t beams_bytes);

/* ---- pictures of a batch: one per scene, all in ONE launch ----
 * The picture of scene i is host/render.js's renderPPM body of what sb_batch_load_scene(i) would return at that point of the
 * stream, byte for byte: RGB8, rows top to bottom, no header -- sb_render's rules, including what is drawn for non-finite
 * coordinates.  A scene never uploaded, or one of zero particles, gives an all-black picture whose bytes ARE written: the output
 * is fully defined, the caller need not clear it.  A render only reads: frame, render, frame equals frame, frame bit for bit,
 * pending break flags included.
 * Zero fields mean: resolution 64; bounds_size and particle_radius those of sb_batch_options; count = every scene from `first` on.
 * sb_batch_render_device only ENQUEUES on the batch's stream: `count` pictures of resolution^2 * 3 bytes, back to back, into
 *   DEVICE memory (no alignment asked for), which must stay valid until that work has run.
 * sb_batch_render_scene WAITS: ONE scene's picture into host memory (debugging, the C user); `first` / `count` are not used.
 * Errors: SB_ERR_INVALID for a NULL handle, a struct_size that is neither 0 nor the struct's, a resolution above
 *   SB_BATCH_RENDER_MAX_RESOLUTION, first or first + count (or `scene`) outside the batch, a NULL output, a host buffer smaller than
 *   the picture -- all checked before anything touches a device; SB_ERR_STATE from sb_batch_render_scene for a scene never
 *   uploaded, as from sb_batch_load_scene. */
#define SB_BATCH_RENDER_MAX_RESOLUTION 1024
typedef struct sb_batch_render_options {
    uint32_t struct_size;    /* = sizeof(sb_batch_render_options); 0 or a NULL pointer = all defaults */
    uint32_t resolution;     /* each picture is resolution x resolution pixels; 0 = 64 */
    double bounds_size;      /* world units across the picture; 0 = sb_batch_options.bounds_size */
    double particle_radius;  /* disc radius in world units; 0 = sb_batch_options.particle_radius */
    uint32_t first, count;   /* scenes first .. first+count-1; count 0 = first .. n_scenes-1 */
    uint32_t reserved[4];
} sb_batch_render_options;
sb_status sb_batch_render_device(sb_batch *b, const sb_batch_render_options *opts, void *device_rgb);
sb_status sb_batch_render_scene(sb_batch *b, uint32_t scene, const sb_batch_render_options *opts, void *rgb, size_t rgb_bytes);

sb_status sb_batch_sync(sb_batch *b);
sb_status sb_batch_get_stream(sb_batch *b, void **hip_stream);
/* key = "n_scenes", "scene_max_particles", "scene_max_beams" (the limits), "max_particles", "max_beams" (this batch's capacity),
 * "threads_per_scene", "lds_bytes_per_scene", "materials_in_lds", "scenes_per_cu", "frame_kernel_vgprs",
 * "frame_kernel_scratch_bytes", "frames_done", "substeps_done", "render_kernel_vgprs", "render_kernel_scratch_bytes",
 * "render_lds_bytes", "render_bands" (the last two: LDS per workgroup and bands per picture of the most recent render);
 * the contact cells of SB_COLLIDE_GRID: "contact_cells_per_side" (G of the G x G grid over the bounds; 0 when the whole batch
 * runs the loop: another mode, a capacity below the threshold, or a radius / bounds whose cell width is no ordinary number),
 * "contact_cell_capacity" (particles a cell holds), "grid_min_particles" (the resolved threshold), and two counts over all
 * scenes and launches so far, which WAIT for the stream: "cell_substeps" (substeps of a scene that ran on the cells) and
 * "cell_overflow_substeps" (substeps of a scene at or above the threshold that ran the loop because a cell was full);
 * "constant_blob_bytes" / "state_blob_bytes" (device memory per scene of what only an upload or a fork writes / of what stepping
 * changes; the latter is kept twice, current and reset); sb_batch_fork_device: "fork_staging_bytes" (device memory of the staging
 * blobs; 0 before the first fork) and, WAITING for the stream, "fork_bad_sources" (entries >= n_scenes other than
 * SB_BATCH_FORK_KEEP seen by all forks so far); sb_batch_summary_device: "summary_words" (SB_BATCH_SUMMARY_WORDS),
 * "summary_kernel_vgprs", "summary_kernel_scratch_bytes"; sb_batch_bodies_device: "body_words" (SB_BATCH_BODY_WORDS),
 * "bodies_kernel_vgprs", "bodies_kernel_scratch_bytes", "bodies_lds_bytes" (LDS of one workgroup at this batch's capacity);
 * sb_batch_contacts_device: "contact_words" (SB_BATCH_CONTACT_WORDS), "contacts_kernel_vgprs", "contacts_kernel_scratch_bytes",
 * "contacts_lds_bytes" (likewise), "contacts_cells_per_side" (G of the G x G cells the call bins into: the rule of
 * "contact_cells_per_side" whatever the collision mode and threshold; 1 where the cell width is no ordinary number);
 * sb_batch_body_summary_device: "body_summary_words" (SB_BATCH_BODY_SUMMARY_WORDS), "body_summary_kernel_vgprs",
 * "body_summary_kernel_scratch_bytes", "body_summary_lds_bytes" (LDS of one workgroup at this batch's capacity);
 * sb_batch_graph_device: "graph_count_words", "graph_material_words", "graph_kernel_vgprs", "graph_kernel_scratch_bytes",
 * "graph_lds_bytes" (likewise); sb_batch_add_particles_device: "add_particles_kernel_vgprs",
 * "add_particles_kernel_scratch_bytes"; sb_batch_raycast_device: "ray_max", "ray_hit_words", "ray_count_words",
 * "raycast_lds_bytes" (likewise), "raycast_kernel_vgprs", "raycast_kernel_scratch_bytes"; sb_batch_nearest_device: "near_max",
 *  "near_hit_words", "near_count_words", "nearest_lds_bytes" (likewise), "nearest_kernel_vgprs", "nearest_kernel_scratch_bytes";
 * sb_batch_forces_device: "force_words", "force_count_words", "forces_lds_bytes" (likewise), "forces_cells_per_side",
 * "forces_kernel_vgprs", "forces_kernel_scratch_bytes"; sb_batch_pose_device: "pose_words" (SB_BATCH_POSE_WORDS),
 * "pose_moment_words" (SB_BATCH_POSE_MOMENT_WORDS), "pose_lds_bytes" (likewise), "pose_kernel_vgprs", "pose_kernel_scratch_bytes" */
sb_status sb_batch_get_info(sb_batch *b, const char *key, uint64_t *value);
const char *sb_batch_last_error(const sb_batch *b);

/* the engine's hipStream_t, so a caller can order its own work (RCCL send/recv) after it. */
sb_status sb_get_stream(sb_engine *e, void **hip_stream);

const char *sb_last_error(const sb_engine *e);
uint32_t sb_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
