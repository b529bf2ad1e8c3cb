"""ctypes binding of the sb_batch_* group of include/softbody.h: N independent small scenes, one workgroup per scene,
one launch per frame.  Like engine.py this only marshals buffers; there is no CPU fallback."""
import collections
import ctypes

import numpy as np

from . import engine as _engine
from .device_binding import DeviceBinding
from .engine import COLLIDE_GRID, EngineError, _ptr
from .layout import LAYOUT_V1, PARTICLE_STRIDE, Buffers

BATCH_MAX_PARTICLES, BATCH_MAX_BEAMS = 1024, 4096     # SB_BATCH_MAX_* (include/softbody.h)
BATCH_RENDER_MAX_RESOLUTION = 1024                    # SB_BATCH_RENDER_MAX_RESOLUTION
FORK_KEEP = 0xFFFFFFFF                                # SB_BATCH_FORK_KEEP: this entry of fork()'s `src` leaves its scene as it is
FORK_CONSTANTS, FORK_AS_RESET = 1, 2                  # SB_BATCH_FORK_*
BEAM_TARGET_LENGTH, BEAM_LAST_LENGTH = 1, 2           # SB_BATCH_BEAM_*
GRID_NEVER = 0xFFFFFFFF                               # sb_batch_options.grid_min_particles: no scene takes the cells
SUMMARY_WORDS = 24                                    # SB_BATCH_SUMMARY_WORDS
# the words of a summary row, in order (include/softbody.h, sb_batch_summary_device): s[:, SUMMARY_FIELDS.index("kinetic_energy")]
SUMMARY_FIELDS = ("particles", "live_beams", "removed_beams", "pending_breaks", "nonfinite_particles", "nonfinite_beams",
                  "mean_x", "mean_y", "mean_vx", "mean_vy", "min_x", "min_y", "max_x", "max_y", "kinetic_energy", "max_speed_sq",
                  "max_strain", "max_stress", "min_stress", "mean_strain", "uploaded", "reserved_21", "reserved_22", "reserved_23")
BODY_WORDS = 4                                        # SB_BATCH_BODY_WORDS
# the words of a row of bodies()'s counts, in order (include/softbody.h, sb_batch_bodies_device)
BODY_FIELDS = ("bodies", "largest_particles", "single_particles", "largest_label")
BODY_SUMMARY_WORDS = 24                               # SB_BATCH_BODY_SUMMARY_WORDS
# the words of a row of body_summary(), in order (include/softbody.h, sb_batch_body_summary_device): SUMMARY_FIELDS' names where the
# word means the same, restricted to the group
BODY_SUMMARY_FIELDS = ("particles", "live_beams", "label", "pending_breaks", "nonfinite_particles", "nonfinite_beams",
                       "mean_x", "mean_y", "mean_vx", "mean_vy", "min_x", "min_y", "max_x", "max_y", "kinetic_energy", "max_speed_sq",
                       "max_strain", "max_stress", "min_stress", "angular_momentum", "reserved_20", "reserved_21", "reserved_22",
                       "reserved_23")
POSE_WORDS, POSE_MOMENT_WORDS = 24, 8                 # SB_BATCH_POSE_WORDS, SB_BATCH_POSE_MOMENT_WORDS
# the words of a row of pose() and of its moments, in order (include/softbody.h, sb_batch_pose_device)
POSE_FIELDS = ("particles", "label", "matched", "unmatched", "mean_x", "mean_y", "ref_mean_x", "ref_mean_y", "mean_vx", "mean_vy",
               "fit_a", "fit_b", "inertia", "ref_inertia", "spin", "angular_velocity", "stretch_sq", "reserved_17", "reserved_18",
               "reserved_19", "reserved_20", "reserved_21", "reserved_22", "reserved_23")
POSE_MOMENT_FIELDS = ("fit_a", "fit_b", "inertia", "ref_inertia", "spin", "matched", "reserved_6", "reserved_7")
# what pose() returns when moments or rank are asked for; None where an output was not asked for
Pose = collections.namedtuple("Pose", ("rows", "moments", "rank"))
# what pose_fit() returns
PoseFit = collections.namedtuple("PoseFit", ("theta", "omega", "rms"))
CONTACT_WORDS = 4                                     # SB_BATCH_CONTACT_WORDS
# the words of a row of contacts()'s touch and of its counts, in order (include/softbody.h, sb_batch_contacts_device)
CONTACT_TOUCH_FIELDS = ("touching", "touching_other_body", "walls", "first_partner")
CONTACT_COUNT_FIELDS = ("pairs", "other_body_pairs", "wall_particles", "touching_particles")
CONTACTS_OTHER_BODY = 1                               # SB_BATCH_CONTACTS_OTHER_BODY
WALL_LEFT, WALL_RIGHT, WALL_LOW, WALL_HIGH = 1, 2, 4, 8   # SB_BATCH_WALL_*: the bits of a touch row's "walls"
ADD_MAX = 64                                          # SB_BATCH_ADD_MAX: rows per scene and call of add_beams()
ADD_ROW_WORDS = 8                                     # sb_batch_new_beam: {a, b, length, spring, damp, yield_strain, strain_break_limit, 0}
ADD_DRY_RUN, ADD_LENGTH_CURRENT, ADD_SKIP_JOINED = 1, 2, 4   # SB_BATCH_ADD_*: the flags
ADD_EMPTY, ADD_INVALID, ADD_JOINED, ADD_FULL = -1, -2, -3, -4   # SB_BATCH_ADD_*: what add_beams()'s result holds where no beam was added
ADD_COUNT_FIELDS = ("added", "invalid", "joined", "full")     # the counts of add_beams(), in order (SB_BATCH_ADD_COUNT_WORDS of them)
SPAWN_ROW_WORDS = 8                                   # sb_batch_new_particle: {tag, x, y, vx, vy, ax, ay, 0}
SPAWN_DRY_RUN, SPAWN_SKIP_TOUCHING = 1, 2             # SB_BATCH_SPAWN_*: the flags
SPAWN_EMPTY, SPAWN_INVALID, SPAWN_BLOCKED, SPAWN_FULL = -1, -2, -3, -4   # SB_BATCH_SPAWN_*: add_particles()'s result where no particle was added
SPAWN_COUNT_FIELDS = ("added", "invalid", "blocked", "full")   # the counts of add_particles(), in order (SB_BATCH_SPAWN_COUNT_WORDS of them)
GRAPH_SKIP_PENDING = 1                                # SB_GRAPH_SKIP_PENDING
GRAPH_COUNT_WORDS, GRAPH_MATERIAL_WORDS = 4, 5        # SB_BATCH_GRAPH_COUNT_WORDS, SB_BATCH_GRAPH_MATERIAL_WORDS
# the words of a row of graph()'s counts and of its material, in order (include/softbody.h, sb_batch_graph_device)
GRAPH_COUNT_FIELDS = ("beams", "connected_particles", "max_degree", "max_degree_particle")
GRAPH_MATERIAL_FIELDS = ("length", "spring", "damp", "yield_strain", "strain_break_limit")
# what graph() returns; None where an output was not asked for
Graph = collections.namedtuple("Graph", ("ends", "material", "row_ptr", "nbr", "counts"))
RAY_MAX = 256                                         # SB_BATCH_RAY_MAX: rays per scene and call of raycast()
RAY_ROW_WORDS = 8                                     # sb_batch_ray: {mask, ox, oy, dx, dy, tmax, skip_label, 0}
RAY_PARTICLES, RAY_BEAMS, RAY_WALLS = 1, 2, 4         # SB_RAY_*: the bits of a row's mask
RAY_MISS, RAY_PARTICLE, RAY_BEAM, RAY_WALL, RAY_EMPTY, RAY_INVALID = 0, 1, 2, 3, -1, -2   # SB_BATCH_RAY_*: the kind of a hit row
RAY_HIT_WORDS, RAY_COUNT_WORDS = 3, 4                 # SB_BATCH_RAY_HIT_WORDS, SB_BATCH_RAY_COUNT_WORDS
# the words of a row of raycast()'s hit and of its counts, in order (include/softbody.h, sb_batch_raycast_device)
RAY_HIT_FIELDS = ("kind", "index", "label")
RAY_COUNT_FIELDS = ("valid", "particles", "beams", "walls")
# what raycast() returns; None where an output was not asked for
RayCast = collections.namedtuple("RayCast", ("t", "hit", "counts"))
NEAR_MAX = 256                                        # SB_BATCH_NEAR_MAX: points per scene and call of nearest()
NEAR_ROW_WORDS = 8                                    # sb_batch_near_point: {mask, px, py, rmax, skip_label, 0, 0, 0}
NEAR_PARTICLES, NEAR_BEAMS, NEAR_WALLS = 1, 2, 4      # SB_NEAR_*: the bits of a row's mask
NEAR_MISS, NEAR_PARTICLE, NEAR_BEAM, NEAR_WALL, NEAR_EMPTY, NEAR_INVALID = 0, 1, 2, 3, -1, -2   # SB_BATCH_NEAR_*: the kind of a hit row
NEAR_HIT_WORDS, NEAR_COUNT_WORDS = 3, 4               # SB_BATCH_NEAR_HIT_WORDS, SB_BATCH_NEAR_COUNT_WORDS
# the words of a row of nearest()'s hit, of its within and of its counts, in order (include/softbody.h, sb_batch_nearest_device)
NEAR_HIT_FIELDS = ("kind", "index", "label")
NEAR_WITHIN_FIELDS = ("particles", "beams")
NEAR_COUNT_FIELDS = ("valid", "particles", "beams", "walls")
# what nearest() returns; None where an output was not asked for
Nearest = collections.namedtuple("Nearest", ("d", "hit", "point", "within", "counts"))
FORCE_WORDS = 8                                       # SB_BATCH_FORCE_WORDS
# the columns of a row of forces(), in order
FORCE_FIELDS = ("beam_x", "beam_y", "push_x", "push_y", "impulse_x", "impulse_y", "depth", "partners")
FORCE_COUNT_FIELDS = ("particles", "beams", "touching_particles", "nonfinite_beams")   # SB_BATCH_FORCE_COUNT_WORDS of them
FORCES_OTHER_BODY = 1                                 # SB_BATCH_FORCES_OTHER_BODY
# what forces() returns; None where an output was not asked for
Forces = collections.namedtuple("Forces", ("rows", "beam_i32", "tension", "counts"))


def new_beam_rows(pairs, spring, damp, yield_strain, strain_break_limit, length=None):
    """Rows for BatchEngine.add_beams() from an int32 torch tensor [N, k, 2] of particle DATA index pairs -- contacts()'s `pairs`
    as it is: a row whose first index is negative stays an empty row -- packed with torch ops on the pairs' device: an int32
    tensor [N, k, 8] in sb_batch_new_beam's layout (the floats as their bits).  spring, damp, yield_strain, strain_break_limit
    and length: a number, or a tensor that broadcasts to [N, k]; length=None fills 0 and is meant for length_current=True."""
    import torch
    if not isinstance(pairs, torch.Tensor) or pairs.dtype != torch.int32 or pairs.dim() != 3 or pairs.shape[2] != 2:
        raise ValueError("new_beam_rows: pairs must be an int32 torch tensor [N, k, 2]")
    n, k = pairs.shape[0], pairs.shape[1]
    rows = torch.zeros((n, k, ADD_ROW_WORDS), dtype=torch.int32, device=pairs.device)
    rows[:, :, 0:2] = pairs
    for col, x in ((2, 0.0 if length is None else length), (3, spring), (4, damp), (5, yield_strain), (6, strain_break_limit)):
        f = torch.as_tensor(x, dtype=torch.float32, device=pairs.device).expand(n, k).contiguous()
        rows[:, :, col] = f.view(torch.int32)
    return rows


def new_particle_rows(pos, vel=None, acc=None, valid=None):
    """Rows for BatchEngine.add_particles() from a float32 torch tensor [N, k, 2] of positions, packed with torch ops on its
    device: an int32 tensor [N, k, 8] in sb_batch_new_particle's layout (the floats as their bits).  vel, acc: float32 tensors that
    broadcast to [N, k, 2], or None for zeros.  valid: a bool tensor that broadcasts to [N, k], False where the row is to be an
    empty one (tag -1); None: every row counts (tag 0)."""
    import torch
    if not isinstance(pos, torch.Tensor) or pos.dtype != torch.float32 or pos.dim() != 3 or pos.shape[2] != 2:
        raise ValueError("new_particle_rows: pos must be a float32 torch tensor [N, k, 2]")
    n, k = pos.shape[0], pos.shape[1]
    rows = torch.zeros((n, k, SPAWN_ROW_WORDS), dtype=torch.int32, device=pos.device)
    for col, x in ((1, pos), (3, vel), (5, acc)):
        if x is not None:
            f = torch.as_tensor(x, dtype=torch.float32, device=pos.device).expand(n, k, 2).contiguous()
            rows[:, :, col:col + 2] = f.view(torch.int32)
    if valid is not None:
        ok = torch.as_tensor(valid, dtype=torch.bool, device=pos.device).expand(n, k)
        rows[:, :, 0] = torch.where(ok, 0, -1).to(torch.int32)
    return rows


def _query_rows(what, first, pairs, floats, ints):
    """The rows of a query (ray_rows, point_rows), packed with torch ops: an int32 tensor [N, k, 8] on the device of `first`, the
    float32 tensor [N, k, 2] that sets N and k (`what`: its name in the error).  pairs: (column, x) with x float32, broadcast to
    [N, k, 2], into two columns as their bits; floats: (column, x) broadcast to [N, k], as their bits; ints: (column, x) integers
    broadcast to [N, k].  The other columns are 0."""
    import torch
    if not isinstance(first, torch.Tensor) or first.dtype != torch.float32 or first.dim() != 3 or first.shape[2] != 2:
        raise ValueError("%s must be a float32 torch tensor [N, k, 2]" % what)
    n, k = first.shape[0], first.shape[1]
    rows = torch.zeros((n, k, RAY_ROW_WORDS), dtype=torch.int32, device=first.device)   # (NEAR_ROW_WORDS is the same 8)
    for col, x in pairs:
        rows[:, :, col:col + 2] = torch.as_tensor(x, dtype=torch.float32, device=first.device).expand(n, k, 2).contiguous().view(torch.int32)
    for col, x in floats:
        rows[:, :, col] = torch.as_tensor(x, dtype=torch.float32, device=first.device).expand(n, k).contiguous().view(torch.int32)
    for col, x in ints:
        rows[:, :, col] = torch.as_tensor(x, device=first.device).to(torch.int32).expand(n, k)
    return rows


def ray_rows(origin, direction, tmax, mask=RAY_PARTICLES | RAY_BEAMS | RAY_WALLS, skip_label=None):
    """Rows for BatchEngine.raycast() from a float32 torch tensor [N, k, 2] of origins, packed with torch ops on its device: an
    int32 tensor [N, k, 8] in sb_batch_ray's layout (the floats as their bits).  direction: a float32 tensor that broadcasts to
    [N, k, 2] (not normalised: t comes back in units of its length).  tmax: a number, or a tensor that broadcasts to [N, k];
    float("inf") is no limit.  mask: RAY_* bits, a number or an integer tensor that broadcasts to [N, k]; 0 makes the row an
    empty one.  skip_label: None (nothing is skipped: -1), a number, or an integer tensor that broadcasts to [N, k] -- a column
    of bodies()'s labels, say."""
    return _query_rows("ray_rows: origin", origin, ((1, origin), (3, direction)), ((5, tmax),), ((0, mask), (6, -1 if skip_label is None else skip_label)))


def point_rows(point, rmax, mask=NEAR_PARTICLES | NEAR_BEAMS | NEAR_WALLS, skip_label=None):
    """Rows for BatchEngine.nearest() from a float32 torch tensor [N, k, 2] of query points, packed with torch ops on its device: an
    int32 tensor [N, k, 8] in sb_batch_near_point's layout (the floats as their bits).  rmax: the reach, a number or a tensor that
    broadcasts to [N, k]; float("inf") is no limit.  mask: NEAR_* bits, a number or an integer tensor that broadcasts to [N, k]; 0
    makes the row an empty one.  skip_label: None (nothing is skipped: -1), a number, or an integer tensor that broadcasts to
    [N, k] -- a column of bodies()'s labels, say."""
    return _query_rows("point_rows: point", point, ((1, point),), ((3, rmax),), ((0, mask), (4, -1 if skip_label is None else skip_label)))


def body_beam_rows(result, edges, length, spring, damp, yield_strain, strain_break_limit):
    """Rows for BatchEngine.add_beams() that join the particles one add_particles() call made into a body: `result` is that
    call's int32 [N, k] (data indices, or negative codes), `edges` an integer tensor [m, 2] of indices into its k rows -- the
    template of the body, the same for every scene.  Returns new_beam_rows()'s format, int32 [N, m, 8], on result's device; a row
    is an empty one wherever either endpoint's result is negative.  length and the material: numbers, or tensors that broadcast
    to [N, m].  Nothing is read back: add_particles -> body_beam_rows -> add_beams spawns a body."""
    import torch
    if not isinstance(result, torch.Tensor) or result.dtype != torch.int32 or result.dim() != 2:
        raise ValueError("body_beam_rows: result must be add_particles()'s int32 torch tensor [N, k]")
    k = result.shape[1]
    on_device = isinstance(edges, torch.Tensor) and edges.is_cuda
    if on_device:
        e = edges
    else:
        host = edges.numpy() if isinstance(edges, torch.Tensor) else edges
        e = torch.as_tensor(np.asarray(host, dtype=np.int64))
    if e.dim() != 2 or e.shape[1] != 2:
        raise ValueError("body_beam_rows: edges must be [m, 2] indices into the %d rows of the spawn call" % k)
    if not on_device and e.numel() and (int(e.min()) < 0 or int(e.max()) >= k):     # (host values: checked here, no read-back)
        raise ValueError("body_beam_rows: edges must be [m, 2] indices into the %d rows of the spawn call" % k)
    e = e.to(device=result.device, dtype=torch.int64)
    # (edges already on the device are not read back: an index outside 0 .. k - 1 makes its row an empty one instead of wrapping)
    outside = ((e < 0) | (e >= k)).any(dim=1)                          # [m]
    pairs = result[:, e.clamp(0, max(k - 1, 0))]                      # [N, m, 2]
    bad = (pairs < 0).any(dim=2, keepdim=True) | outside[None, :, None]
    pairs = torch.where(bad, torch.full_like(pairs, -1), pairs)
    return new_beam_rows(pairs.contiguous(), spring, damp, yield_strain, strain_break_limit, length=length)


def pose_fit(moments):
    """Angle, angular velocity and misfit from BatchEngine.pose()'s `moments` (float64 [..., POSE_MOMENT_WORDS]): a PoseFit of
    float64 tensors [...] on the moments' device --
      theta = atan2(b, a)      the rotation that best carries the reference onto the current shape,
      omega = Lc / I           the angular velocity,
      rms   = sqrt(max(I + I0 - 2 sqrt(a^2 + b^2), 0) / n)   the root-mean-square distance left after the best rigid fit.
    Plain torch float64: unlike the moments these are NOT pinned bit for bit (sqrt and atan2 are the device library's).  A row
    without a matched member gives NaN."""
    import torch
    if not isinstance(moments, torch.Tensor) or moments.dtype != torch.float64 or moments.shape[-1] != POSE_MOMENT_WORDS:
        raise ValueError("pose_fit: moments must be pose()'s float64 torch tensor [..., %d]" % POSE_MOMENT_WORDS)
    a, b, inertia, ref_inertia, spin, n = (moments[..., k] for k in range(6))
    rest = torch.clamp(inertia + ref_inertia - 2.0 * torch.sqrt(a * a + b * b), min=0.0)
    return PoseFit(torch.atan2(b, a), spin / inertia, torch.sqrt(rest / n))


class SbBatchOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_scenes", ctypes.c_uint32), ("bounds_size", ctypes.c_float),
                ("particle_radius", ctypes.c_float), ("subticks", ctypes.c_uint32), ("max_particles", ctypes.c_uint32),
                ("max_beams", ctypes.c_uint32), ("layout", ctypes.c_uint32), ("collision_mode", ctypes.c_uint32),
                ("device_ordinal", ctypes.c_int32), ("grid_min_particles", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 5)]


class SbBatchRenderOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("resolution", ctypes.c_uint32), ("bounds_size", ctypes.c_double),
                ("particle_radius", ctypes.c_double), ("first", ctypes.c_uint32), ("count", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 4)]


_bound = None


def load_library():
    """engine.load_library() (which checks that every declared symbol is exported) plus the prototypes of sb_batch_*."""
    global _bound
    if _bound is not None:
        return _bound
    L = _engine.load_library()
    vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    L.sb_batch_default_options.argtypes = [ctypes.POINTER(SbBatchOptions)]
    L.sb_batch_default_options.restype = None
    L.sb_batch_create.argtypes = [ctypes.POINTER(SbBatchOptions), ctypes.POINTER(vp)]
    L.sb_batch_destroy.argtypes = [vp]
    L.sb_batch_write_scene.argtypes = [vp, u32, u32, vp, sz, vp, sz, vp, sz, vp, sz]
    L.sb_batch_write_user_input.argtypes = [vp, vp]
    L.sb_batch_write_user_input_device.argtypes = [vp, vp]
    L.sb_batch_set_physics_constants.argtypes = [vp, u32, u32, vp]
    L.sb_batch_frame.argtypes = [vp, u32]
    L.sb_batch_step.argtypes = [vp, u32]
    L.sb_batch_delete_pass.argtypes = [vp]
    L.sb_batch_reset_device.argtypes = [vp, vp]
    L.sb_batch_read_state_device.argtypes = [vp, vp, vp, vp]
    L.sb_batch_write_particles_device.argtypes = [vp, vp]
    L.sb_batch_fork_device.argtypes = [vp, vp, u32]
    L.sb_batch_checkpoint_device.argtypes = [vp, vp]
    L.sb_batch_write_beams_device.argtypes = [vp, vp, u32]
    L.sb_batch_cut_device.argtypes = [vp, u32, vp, u32, vp, vp]
    L.sb_batch_add_beams_device.argtypes = [vp, u32, vp, u32, vp, vp]
    L.sb_batch_add_particles_device.argtypes = [vp, u32, vp, u32, vp, vp]
    L.sb_batch_summary_device.argtypes = [vp, vp]
    L.sb_batch_rollout_device.argtypes = [vp, u32, vp, vp]
    L.sb_batch_bodies_device.argtypes = [vp, vp, vp, vp]
    L.sb_batch_contacts_device.argtypes = [vp, u32, vp, vp, vp, u32, vp]
    L.sb_batch_graph_device.argtypes = [vp, u32, vp, vp, vp, vp, vp]
    L.sb_batch_raycast_device.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp]
    L.sb_batch_nearest_device.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp, vp, vp]
    L.sb_batch_forces_device.argtypes = [vp, u32, vp, vp, vp, vp, vp]
    L.sb_batch_body_summary_device.argtypes = [vp, vp, u32, vp, vp]
    L.sb_batch_pose_device.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    L.sb_batch_load_scene.argtypes = [vp, u32, vp, sz, vp, sz, vp, sz, vp, sz]
    L.sb_batch_render_device.argtypes = [vp, ctypes.POINTER(SbBatchRenderOptions), vp]
    L.sb_batch_render_scene.argtypes = [vp, u32, ctypes.POINTER(SbBatchRenderOptions), vp, sz]
    L.sb_batch_sync.argtypes = [vp]
    L.sb_batch_get_stream.argtypes = [vp, ctypes.POINTER(vp)]
    L.sb_batch_get_info.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
    L.sb_batch_last_error.argtypes = [vp]
    L.sb_batch_last_error.restype = ctypes.c_char_p
    for name in _engine.declared_symbols():
        if name.startswith("sb_batch_") and name not in ("sb_batch_default_options", "sb_batch_last_error"):
            getattr(L, name).restype = ctypes.c_int
    _bound = L
    return L


class BatchEngine(DeviceBinding):
    """N independent scenes of at most BATCH_MAX_PARTICLES particles / BATCH_MAX_BEAMS beams each, stepped together.
    max_particles / max_beams are the capacity PER SCENE (the sizes of the layout.Buffers that write_scene / load_scene take).

    collision_mode: COLLIDE_OFF, COLLIDE_ALLPAIRS (the reference's loop over every slot) or COLLIDE_GRID (the default): scenes
    of at least `grid_min_particles` particles bin their particles into a cell grid in LDS every substep and test only the
    3 x 3 cells around each particle -- the same bits as COLLIDE_ALLPAIRS.  grid_min_particles: None / 0 = the build's default
    (the measured break-even), n = 1 .. BATCH_MAX_PARTICLES, GRID_NEVER = no scene.
    info() keys of the cells: "contact_cells_per_side" (0: the whole batch runs the loop), "contact_cell_capacity",
    "grid_min_particles" (resolved), and, waiting for the stream, "cell_substeps" (scene-substeps that ran on the cells) and
    "cell_overflow_substeps" (scene-substeps that ran the loop because a cell held more than its capacity)."""

    _owner = "batch"

    def __init__(self, n_scenes=1, bounds_size=1000.0, particle_radius=10.0, subticks=64, layout=LAYOUT_V1,
                 max_particles=BATCH_MAX_PARTICLES, max_beams=BATCH_MAX_BEAMS, collision_mode=COLLIDE_GRID, device=0,
                 grid_min_particles=None):
        L = load_library()
        o = SbBatchOptions()
        L.sb_batch_default_options(ctypes.byref(o))
        o.n_scenes, o.bounds_size, o.particle_radius, o.subticks = n_scenes, bounds_size, particle_radius, subticks
        o.max_particles, o.max_beams, o.layout = max_particles, max_beams, layout
        o.collision_mode, o.device_ordinal = collision_mode, device
        o.grid_min_particles = 0 if grid_min_particles is None else grid_min_particles
        self._h = ctypes.c_void_p()
        st = L.sb_batch_create(ctypes.byref(o), ctypes.byref(self._h))
        if st != 0:
            self._h = None
            raise EngineError(st, L.sb_batch_last_error(None).decode())
        self.n_scenes, self.layout, self.max_particles, self.max_beams = n_scenes, layout, max_particles, max_beams
        self.device, self.collision_mode = device, collision_mode
        self.subticks = (subticks + 1) // 2 * 2
        self._ext_stream = None

    def _check(self, st):
        if st != 0:
            raise EngineError(st, load_library().sb_batch_last_error(self._h).decode())

    def destroy(self):
        if self._h:
            load_library().sb_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # ---- scenes in and out (host buffers)
    def write_scene(self, buf: Buffers, first=0, count=None):
        """Upload ONE scene into scenes first .. first+count-1 (count=None: all scenes from `first` on); it also becomes
        their reset state.  Waits for the stream."""
        count = self.n_scenes - first if count is None else count
        self._check(load_library().sb_batch_write_scene(
            self._h, first, count, _ptr(buf.metadata), buf.metadata.nbytes, _ptr(buf.mapping), buf.mapping.nbytes,
            _ptr(buf.particles), buf.particles.nbytes, _ptr(buf.beams), buf.beams.nbytes))

    def load_scene(self, i, buf: Buffers):
        """Scene i into `buf` exactly as Engine.load_buffers returns a single engine in the same state.  Waits."""
        self._check(load_library().sb_batch_load_scene(
            self._h, i, _ptr(buf.metadata), buf.metadata.nbytes, _ptr(buf.mapping), buf.mapping.nbytes,
            _ptr(buf.particles), buf.particles.nbytes, _ptr(buf.beams), buf.beams.nbytes))
        return buf

    # ---- inputs
    def write_user_input(self, x):
        """32 bytes (bytes / bytearray / numpy): every scene gets them; or a contiguous torch tensor of n_scenes x 32 bytes on
        the batch's device (any dtype, e.g. float32 [n_scenes, 8] with mouse_active's bits in column 1): scene i gets row i."""
        if isinstance(x, (bytes, bytearray, memoryview, np.ndarray)):
            raw = bytes(x.tobytes() if isinstance(x, np.ndarray) else x)
            if len(raw) != 32:
                raise ValueError("write_user_input: 32 bytes are needed, not %d" % len(raw))
            b = (ctypes.c_ubyte * 32).from_buffer_copy(raw)
            return self._check(load_library().sb_batch_write_user_input(self._h, ctypes.cast(b, ctypes.c_void_p)))
        ptr, t = self._device_buffer("write_user_input", x, None, self.n_scenes * 32)
        self._ordered(t, lambda: load_library().sb_batch_write_user_input_device(self._h, ctypes.c_void_p(ptr)))

    def set_physics_constants(self, consts8, first=0, count=None):
        a = np.ascontiguousarray(consts8, dtype="<f4")
        if a.shape != (8,):
            raise ValueError("set_physics_constants: 8 floats are needed")
        count = self.n_scenes - first if count is None else count
        self._check(load_library().sb_batch_set_physics_constants(self._h, first, count, _ptr(a)))

    # ---- stepping (only enqueues)
    def frame(self, n=1):
        self._check(load_library().sb_batch_frame(self._h, n))

    def step(self, n):
        self._check(load_library().sb_batch_step(self._h, n))

    def delete_pass(self):
        self._check(load_library().sb_batch_delete_pass(self._h))

    def reset(self, mask=None):
        """Scenes whose mask entry is nonzero (a uint8 / bool torch tensor of n_scenes entries on the device, or a device
        pointer) go back to their reset state: their latest upload, or a later checkpoint() / fork(); None = all."""
        if mask is None:
            return self._check(load_library().sb_batch_reset_device(self._h, None))
        ptr, t = self._device_buffer("reset", mask, ("uint8", "bool"), self.n_scenes)
        self._ordered(t, lambda: load_library().sb_batch_reset_device(self._h, ctypes.c_void_p(ptr)))

    def checkpoint(self, mask=None):
        """The inverse of reset(): scenes whose mask entry is nonzero (as in reset(); None = all) make their CURRENT state their
        reset state -- particles, beam state, beam mapping, live-beam count, pending break flags, removed beams.  Scenes never
        uploaded are skipped.  Only enqueues."""
        if mask is None:
            return self._check(load_library().sb_batch_checkpoint_device(self._h, None))
        ptr, t = self._device_buffer("checkpoint", mask, ("uint8", "bool"), self.n_scenes)
        self._ordered(t, lambda: load_library().sb_batch_checkpoint_device(self._h, ctypes.c_void_p(ptr)))

    def fork(self, src, constants=False, as_reset=False):
        """Scene i becomes a copy of scene src[i]: `src` is an int32 / uint32 torch tensor of n_scenes entries on the device (or a
        device pointer to as many 32-bit words).  Every source is read as it was before the call, so permutations, swaps and a
        broadcast from a scene that is itself overwritten are well defined.  src[i] == i and FORK_KEEP (-1 in an int32 tensor)
        leave scene i as it is; so does any other entry outside the batch, counted in info("fork_bad_sources").
        Copied: topology and materials, particles, beam state, beam mapping, counts, pending break flags, removed beams.  The
        destination keeps its user input and, unless constants=True, its physics constants.  Its reset state becomes the
        source's (reset() then takes it where it would take the source), or, with as_reset=True, the forked state itself.  A
        source never uploaded makes the destination a never-uploaded scene.  Only enqueues; the first fork allocates the
        staging blobs (info("fork_staging_bytes"))."""
        ptr, t = self._device_buffer("fork", src, ("int32", "uint32"), self.n_scenes * 4)
        if t and src.numel() != self.n_scenes:
            raise ValueError("fork: one source per scene is needed (%d), not %d" % (self.n_scenes, src.numel()))
        flags = (FORK_CONSTANTS if constants else 0) | (FORK_AS_RESET if as_reset else 0)
        self._ordered(t, lambda: load_library().sb_batch_fork_device(self._h, ctypes.c_void_p(ptr), flags))

    def sync(self):
        self._check(load_library().sb_batch_sync(self._h))

    def info(self, key):
        v = ctypes.c_uint64()
        self._check(load_library().sb_batch_get_info(self._h, key.encode(), ctypes.byref(v)))
        return v.value

    def stream(self):
        s = ctypes.c_void_p()
        self._check(load_library().sb_batch_get_stream(self._h, ctypes.byref(s)))
        return s.value

    # ---- the state in device memory
    def read_state_device(self, particles=None, beams=None, beam_alive=None):
        """Engine.read_state_device with a leading scene dimension: particles float32 [n_scenes, max_particles, 6], beams
        float32 [n_scenes, max_beams, 4] {target_length, last_length, strain, stress}, beam_alive uint8 / bool
        [n_scenes, max_beams], each at DATA indices; rows of no particle / beam are not written.  Only enqueues."""
        n, args, tensors = self.n_scenes, [], False
        for what, x, dtype, nb in (("particles", particles, "float32", n * self.max_particles * PARTICLE_STRIDE),
                                   ("beams", beams, "float32", n * self.max_beams * 16),
                                   ("beam_alive", beam_alive, ("uint8", "bool"), n * self.max_beams)):
            if x is None:
                args.append(None)
                continue
            ptr, t = self._device_buffer("read_state_device: " + what, x, dtype, nb)
            args.append(ptr)
            tensors |= t
        vp = ctypes.c_void_p
        self._ordered(tensors, lambda: load_library().sb_batch_read_state_device(self._h, vp(args[0]), vp(args[1]), vp(args[2])))

    def write_particles_device(self, src):
        """Overwrite p, v, a of every particle of every scene from float32 [n_scenes, max_particles, 6] on the device (only
        rows of a scene's particles are read).  Beams, counts, mappings and pending break flags are untouched."""
        ptr, t = self._device_buffer("write_particles_device", src, "float32", self.n_scenes * self.max_particles * PARTICLE_STRIDE)
        self._ordered(t, lambda: load_library().sb_batch_write_particles_device(self._h, ctypes.c_void_p(ptr)))

    def write_beams_device(self, src, target_length=True, last_length=False):
        """The counterpart of write_particles_device for beams: `src` is float32 [n_scenes, max_beams, 4] on the device in
        read_state_device's beam layout; target_length / last_length select which of the first two floats of every row are
        written (strain and stress never are).  Only rows of beams of a scene's latest upload are read; a removed beam's row is
        written but inert.  Counts, mappings, removed beams and pending break flags are untouched.  Only enqueues."""
        fields = (BEAM_TARGET_LENGTH if target_length else 0) | (BEAM_LAST_LENGTH if last_length else 0)
        ptr, t = self._device_buffer("write_beams_device", src, "float32", self.n_scenes * self.max_beams * 16)
        self._ordered(t, lambda: load_library().sb_batch_write_beams_device(self._h, ctypes.c_void_p(ptr), fields))

    def state_tensors(self):
        """(particles [N, maxP, 6] float32, beams [N, maxB, 4] float32, alive [N, maxB] bool) of the current state as new torch
        tensors; rows of no particle / beam are NaN (False in alive)."""
        import torch
        dev = torch.device("cuda", self.device)
        p = torch.full((self.n_scenes, self.max_particles, 6), float("nan"), dtype=torch.float32, device=dev)
        b = torch.full((self.n_scenes, self.max_beams, 4), float("nan"), dtype=torch.float32, device=dev)
        a = torch.zeros((self.n_scenes, self.max_beams), dtype=torch.bool, device=dev)
        self.read_state_device(p, b, a)
        return p, b, a

    # ---- per-scene statistics and rollouts (sb_batch_summary_device / sb_batch_rollout_device)
    def summary(self, out=None):
        """One row of SUMMARY_WORDS statistics per scene (SUMMARY_FIELDS names the columns) in one launch: a float32 tensor
        [n_scenes, 24] on the batch's device -- counts, means, extremes and the kinetic energy of the finite particles, strain
        and stress of the finite live beams; an empty set gives NaN; every word is written.  `out`: a device pointer (int) or a
        contiguous float32 torch tensor of at least n_scenes * 24 elements to write into.  Only reads the batch, only enqueues;
        torch's current stream is ordered after it."""
        (out,), (ptr,), t = self._bind("summary", [("out", out, True, (self.n_scenes, SUMMARY_WORDS), "float32")])
        self._ordered(t, lambda: load_library().sb_batch_summary_device(self._h, ctypes.c_void_p(ptr)))
        return out

    def rollout(self, inputs=None, frames=None, summary=True, out=None):
        """`frames` times: (scene i gets the 32 bytes inputs[t, i] as write_user_input would write them), frame(), (summary()
        into row t) -- enqueued in one call, bit for bit what the individual calls give.  inputs: a device pointer (int) or a
        contiguous torch tensor of frames x n_scenes x 32 bytes on the batch's device (any dtype, e.g. float32 [T, N, 8]);
        None: the inputs stay as they are.  frames: None = inputs.shape[0]; required when `inputs` is None or a pointer.
        Returns a float32 tensor [frames, n_scenes, 24] (`out`: a pointer or a float32 tensor of at least that many elements to
        write into), or None with summary=False.  Afterwards the scenes hold the inputs of the last slice."""
        import torch
        n = self.n_scenes
        if frames is None:
            if not isinstance(inputs, torch.Tensor) or inputs.dim() == 0:
                raise ValueError("rollout: `frames` is needed when `inputs` is not a tensor with a leading frame dimension")
            frames = inputs.shape[0]
        frames = int(frames)
        if frames < 0:
            raise ValueError("rollout: frames is %d" % frames)
        iptr, tensors = None, False
        if inputs is not None:
            iptr, tensors = self._device_buffer("rollout: inputs", inputs, None, frames * n * 32)
        if not summary and out is not None:
            raise ValueError("rollout: `out` is given but summary=False")
        (out,), (optr,), t = self._bind("rollout", [("out", out, bool(summary), (frames, n, SUMMARY_WORDS), "float32")])
        vp = ctypes.c_void_p
        self._ordered(tensors | t, lambda: load_library().sb_batch_rollout_device(self._h, frames, vp(iptr), vp(optr)))
        return out

    # ---- connected bodies (sb_batch_bodies_device)
    def bodies(self, labels=None, sizes=False, counts=None):
        """The connected bodies of every scene in one launch: particles joined by LIVE beams (a pending break flag still
        connects, a beam removed by a delete pass does not).  Returns (labels, counts), int32 tensors on the batch's device, or
        (labels, counts, sizes) with sizes=True or a tensor.  labels [n_scenes, max_particles]: at particle DATA index i (the rows
        of read_state_device) the smallest data index of i's body, -1 where no particle lives -- what torch.index_add_ takes for a
        statistic per body.  counts [n_scenes, 4] (BODY_FIELDS names the columns): bodies, particles of the largest, bodies of one
        particle, label of the largest (the smallest label on a tie; -1 in a scene of no particles or never uploaded).  sizes
        [n_scenes, max_particles, 2]: {particles, live beams} of the body at its label's row, {0, 0} in every other row.  Every
        word is written.  labels / counts / sizes: a device pointer (int) or a contiguous int32 torch tensor of at least that
        many elements to write into.  Only reads the batch, only enqueues; torch's current stream is ordered after it."""
        n, maxp = self.n_scenes, self.max_particles
        given = [None if x is True else x for x in (labels, None if sizes is False else sizes, counts)]   # (True: a new tensor)
        outs, ptrs, tensors = self._bind("bodies", [("labels", given[0], True, (n, maxp), "int32"),
                                                    ("sizes", given[1], sizes is not False, (n, maxp, 2), "int32"),
                                                    ("counts", given[2], True, (n, BODY_WORDS), "int32")])
        vp = ctypes.c_void_p
        self._ordered(tensors, lambda: load_library().sb_batch_bodies_device(self._h, vp(ptrs[0]), vp(ptrs[1]), vp(ptrs[2])))
        return (outs[0], outs[2], outs[1]) if sizes is not False else (outs[0], outs[2])

    # ---- cutting beams (sb_batch_cut_device)
    def cut(self, shapes, dry_run=False, hit=False, counts=None):
        """Cut every scene with its own k shapes in one launch: `shapes` is [n_scenes, k, 8] (engine.cut_shapes packs rows:
        {kind, x0, y0, x1, y1, 0, 0, 0}; CUT_SEGMENT: a knife from (x0, y0) to (x1, y1); CUT_DISC: an eraser at (x0, y0) of radius
        x1; CUT_NONE: ignored), k <= 64 -- an int32 torch tensor on the batch's device (the coordinates as float bits), a float32
        tensor (the kind as a number: converted on the device), or a numpy array / nested list, which is uploaded.  Every live
        beam a shape hits (include/softbody.h states the predicate) gets its pending break flag raised: the next frame's delete
        pass removes it; reset() undoes it, fork() copies it, checkpoint() keeps it.  dry_run: report only.  Returns (hit, counts):
        hit uint8 [n_scenes, max_beams], 1 at the DATA index of a hit beam, else 0 (hit=True or a tensor / pointer; None
        otherwise); counts int32 [n_scenes, 4] (CUT_COUNT_FIELDS: tested, hit, flagged, already_flagged; counts=False: None).
        A scene never uploaded, or whose shapes are all CUT_NONE, is untouched.  Only enqueues."""
        from .engine import CUT_DRY_RUN, CUT_MAX_SHAPES, CUT_COUNT_FIELDS, device_shapes
        import torch
        n = self.n_scenes
        words = device_shapes(shapes, torch.device("cuda", self.device), 3)
        if words.shape[0] != n or words.shape[1] > CUT_MAX_SHAPES:
            raise ValueError("cut: shapes must be [n_scenes = %d, k <= %d, 8], not %s" % (n, CUT_MAX_SHAPES, tuple(words.shape)))
        k = int(words.shape[1])
        given = [None if isinstance(x, bool) else x for x in (hit, counts)]   # (True: a new tensor)
        outs, ptrs, tensors = self._bind("cut", [("hit", given[0], hit is not False, (n, self.max_beams), "uint8"),
                                                 ("counts", given[1], counts is not False, (n, len(CUT_COUNT_FIELDS)), "int32")])
        vp = ctypes.c_void_p
        self._ordered(True, lambda: load_library().sb_batch_cut_device(self._h, CUT_DRY_RUN if dry_run else 0, vp(words.data_ptr() if k else None),
                                                                       k, vp(ptrs[0]), vp(ptrs[1])))
        return outs[0], outs[1]

    # ---- adding beams (sb_batch_add_beams_device)
    def add_beams(self, rows, *, length_current=False, skip_joined=False, dry_run=False, result=None, counts=None):
        """The inverse of cut(): every scene gets its own k new beams ("welds") in one launch.  `rows` is [n_scenes, k, 8],
        k <= ADD_MAX, in sb_batch_new_beam's layout {a, b, length, spring, damp, yield_strain, strain_break_limit, 0} -- a and b
        particle DATA indices as integers, the five floats as their bits: an int32 or float32 (bits) torch tensor on the batch's
        device (new_beam_rows() packs one from contacts()'s pairs), or a tuple (device pointer, k).
        include/softbody.h states the rule row by row: a < 0 is an empty row; a row that names no two particles of the scene, has
        a nonzero last word or a length that is no finite number > 0 is ADD_INVALID; with skip_joined a pair that a live beam or
        an earlier row of the call already joins is ADD_JOINED; a row that finds no free beam slot or data index is ADD_FULL.
        length_current: the rest length is the endpoints' current distance.  dry_run: report only.  Returns (result, counts):
        result int32 [n_scenes, k], the new beam's DATA index or the code; counts int32 [n_scenes, 4] (ADD_COUNT_FIELDS).  An
        added beam is from then on a beam of the scene as if uploaded; checkpoint() keeps it, reset() removes it, fork() copies
        it.  result / counts: a device pointer (int) or a contiguous int32 torch tensor to write into.  Only enqueues."""
        flags = (ADD_DRY_RUN if dry_run else 0) | (ADD_LENGTH_CURRENT if length_current else 0) | (ADD_SKIP_JOINED if skip_joined else 0)
        return self._add_rows("add_beams", load_library().sb_batch_add_beams_device, rows, ADD_ROW_WORDS, flags, result, counts, ADD_COUNT_FIELDS)

    # ---- adding particles (sb_batch_add_particles_device)
    def add_particles(self, rows, *, skip_touching=False, dry_run=False, result=None, counts=None):
        """Every scene gets its own k new particles ("spawns") in one launch.  `rows` is [n_scenes, k, 8], k <= ADD_MAX, in
        sb_batch_new_particle's layout {tag, x, y, vx, vy, ax, ay, 0} -- the tag an integer, the six floats as their bits: an int32
        or float32 (bits) torch tensor on the batch's device (new_particle_rows() packs one), or a tuple (device pointer, k).
        include/softbody.h states the rule row by row: tag < 0 is an empty row; a row with a nonzero last word, or whose x or y
        is not finite, or in a scene never uploaded, is SPAWN_INVALID; with skip_touching a row that touches a particle of the
        scene (contacts()'s test), or an earlier row of the call that itself touches none, is SPAWN_BLOCKED; a row that finds no
        free particle slot or data index is SPAWN_FULL.  dry_run: report only.  Returns (result, counts): result int32
        [n_scenes, k], the new particle's DATA index -- what a row of add_beams() names -- or the code; counts int32 [n_scenes, 4]
        (SPAWN_COUNT_FIELDS).  An added particle is from then on a particle of the scene as if uploaded; checkpoint() keeps it,
        reset() removes it together with every beam welded onto it, fork() copies it.  result / counts: a device pointer (int)
        or a contiguous int32 torch tensor to write into.  Only enqueues."""
        flags = (SPAWN_DRY_RUN if dry_run else 0) | (SPAWN_SKIP_TOUCHING if skip_touching else 0)
        return self._add_rows("add_particles", load_library().sb_batch_add_particles_device, rows, SPAWN_ROW_WORDS, flags, result, counts,
                              SPAWN_COUNT_FIELDS)

    def _add_rows(self, what, entry, rows, row_words, flags, result, counts, count_fields):
        """add_beams() / add_particles() (`what`: the name in the messages, `entry`: its function of the library): k rows of
        row_words words per scene in, (result [n_scenes, k], counts [n_scenes, len(count_fields)]) out"""
        import torch
        n = self.n_scenes
        if isinstance(rows, tuple):
            ptr, k = int(rows[0]), int(rows[1])
            is_tensor = False
        else:
            if not isinstance(rows, torch.Tensor) or rows.dtype not in (torch.int32, torch.float32):
                raise ValueError("%s: rows must be an int32 / float32 torch tensor [n_scenes, k, 8] or (device pointer, k)" % what)
            if rows.dim() != 3 or rows.shape[0] != n or rows.shape[2] != row_words or rows.shape[1] > ADD_MAX:
                raise ValueError("%s: rows must be [n_scenes = %d, k <= %d, 8], not %s" % (what, n, ADD_MAX, tuple(rows.shape)))
            k = int(rows.shape[1])
            ptr, is_tensor = self._device_buffer(what + ": rows", rows, None, n * k * row_words * 4)
        if not 0 <= k <= ADD_MAX:
            raise ValueError("%s: k is %d, not in 0 .. %d" % (what, k, ADD_MAX))
        outs, ptrs, tensors = self._bind(what, [("result", result, True, (n, k), "int32"),
                                                ("counts", counts, True, (n, len(count_fields)), "int32")])
        vp = ctypes.c_void_p
        self._ordered(tensors or is_tensor, lambda: entry(self._h, flags, vp(ptr if k else None), k, vp(ptrs[0]), vp(ptrs[1])))
        return outs[0], outs[1]

    # ---- statistics per body (sb_batch_body_summary_device)
    def body_summary(self, labels=None, rows=8, out=None, rank=False):
        """One row of BODY_SUMMARY_WORDS statistics per GROUP of particles of every scene in one launch (BODY_SUMMARY_FIELDS names
        the columns): a float32 tensor [n_scenes, rows, 24] on the batch's device, or (that, rank) with rank=True or a tensor.
        labels: None (self.bodies() is called first, on the same stream, and the groups are the bodies) or an int32 tensor /
        device pointer of [n_scenes, max_particles] labels of the caller's own at particle DATA indices: a value 0 .. max_particles-1
        names the particle's group, any other value puts it into none; a live beam belongs to the group that holds both its
        endpoints.  Row k of a scene is its group of rank k -- particles descending, then label ascending -- and rows behind the
        last group are empty (label -1, counts 0, NaN elsewhere).  Counts, label, pending breaks, means, extremes, kinetic energy
        and angular momentum of the group's finite particles, strain and stress extremes of its finite beams; the sums are those
        of summary()'s pinned tree over the group alone, so a row is reproducible bit for bit, and a scene that is one body gives
        summary()'s words.  rank int32 [n_scenes, max_particles]: the rank of the group of the particle at that data index (>= rows:
        its row was cut), -1 where no particle lives or the particle is in no group.  rows: 1 .. max_particles.  out / rank: a
        device pointer (int) or a contiguous torch tensor (float32 / int32) of at least that many elements to write into.  Every
        word is written.  Only reads the batch, only enqueues; torch's current stream is ordered after it."""
        n, maxp = self.n_scenes, self.max_particles
        if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or not 1 <= rows <= maxp:
            raise ValueError("body_summary: rows is %r, not a number in 1 .. max_particles (%d)" % (rows, maxp))
        rows = int(rows)
        outs, ptrs, tensors = self._bind("body_summary", [
            ("out", None if out is True else out, True, (n, rows, BODY_SUMMARY_WORDS), "float32"),
            ("rank", None if rank is True or rank is False else rank, rank is not False, (n, maxp), "int32"),
            ("labels", (lambda: self.bodies()[0]) if labels is None else labels, True, (n, maxp), "int32")])
        vp = ctypes.c_void_p
        self._ordered(tensors, lambda: load_library().sb_batch_body_summary_device(self._h, vp(ptrs[2]), rows, vp(ptrs[0]), vp(ptrs[1])))
        return (outs[0], outs[1]) if rank is not False else outs[0]

    # ---- pose per body against a reference shape (sb_batch_pose_device)
    def pose(self, labels=None, ref=None, rows=8, out=None, moments=False, rank=False):
        """How every GROUP of particles of every scene is turned, how fast it spins and how far it is bent out of shape, in one
        launch: a float32 tensor [n_scenes, rows, POSE_WORDS] on the batch's device (POSE_FIELDS names the columns), or, with
        moments or rank asked for, a Pose (rows, moments, rank) with None where an output was not.  labels, rows, rank and the
        ranking are body_summary()'s: labels=None calls self.bodies() first, on the same stream, and the groups are the bodies;
        row k is the group of rank k -- the group of body_summary()'s row k.  ref: None -- every particle is compared with its
        position in the scene's RESET state (the latest write_scene / checkpoint / fork; it never leaves the device), and a
        particle spawned since then has no reference until a checkpoint() -- or a float32 tensor / device pointer
        [n_scenes, max_particles, 2] of reference positions {X, Y} at particle DATA indices (a NaN row: no reference).  A member is
        matched when its record is finite and it has a finite reference; a row holds particles, label, matched, unmatched, then
        over the matched members the current centroid, the reference's centroid, the mean velocity, the fit's a and b (the rotation
        from the reference to the current shape is atan2(b, a)), the moments of inertia of the current and of the reference shape
        about their centroids, the spin (angular momentum about the centroid), the angular velocity spin / inertia and the squared
        stretch inertia / ref_inertia; NaN where nothing is matched.  moments (True or a tensor / pointer): float64
        [n_scenes, rows, POSE_MOMENT_WORDS] {a, b, I, I0, Lc, n, 0, 0} (POSE_MOMENT_FIELDS), what pose_fit() takes.  The sums are
        those of summary()'s pinned tree over the matched members, in double, and what derives from them uses + - * / alone, so
        rows and moments are reproducible bit for bit: an argmin over them does not flip.  out / moments / rank: a device
        pointer (int) or a contiguous torch tensor (float32 / float64 / int32) of at least that many elements to write into.
        Every word is written.  Only reads the batch, only enqueues; torch's current stream is ordered after it.

        Upright reward, nothing exported:
            r = be.pose()                                        # against the reset state, per body
            upright = torch.cos(torch.atan2(r[:, 0, 11], r[:, 0, 10]))
        Match this target shape (target: float32 [n_scenes, max_particles, 2] at data indices):
            p = be.pose(ref=target, moments=True)
            cost = pose_fit(p.moments).rms[:, 0]                # 0 where the largest body is the target, turned and shifted"""
        n, maxp = self.n_scenes, self.max_particles
        if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or not 1 <= rows <= maxp:
            raise ValueError("pose: rows is %r, not a number in 1 .. max_particles (%d)" % (rows, maxp))
        rows = int(rows)
        outs, ptrs, tensors = self._bind("pose", [
            ("out", None if out is True else out, True, (n, rows, POSE_WORDS), "float32"),
            ("moments", None if moments is True or moments is False else moments, moments is not False, (n, rows, POSE_MOMENT_WORDS), "float64"),
            ("rank", None if rank is True or rank is False else rank, rank is not False, (n, maxp), "int32"),
            ("ref", ref, ref is not None, (n, maxp, 2), "float32"),
            ("labels", (lambda: self.bodies()[0]) if labels is None else labels, True, (n, maxp), "int32")])
        vp = ctypes.c_void_p
        self._ordered(tensors, lambda: load_library().sb_batch_pose_device(self._h, vp(ptrs[4]), vp(ptrs[3]), rows, vp(ptrs[0]), vp(ptrs[1]),
                                                                           vp(ptrs[2])))
        return Pose(outs[0], outs[1], outs[2]) if moments is not False or rank is not False else outs[0]

    # ---- particle and wall contacts (sb_batch_contacts_device)
    def contacts(self, labels=None, pairs=0, other_body=False, touch=None, counts=None):
        """Who touches whom, and who touches a wall, in every scene in one launch.  Two particles touch iff the next substep's
        collision loop would act on them (dist == 0 or dist < 2 * particle_radius in the library's float arithmetic); the answer
        is the same in every collision_mode, COLLIDE_OFF included.  Returns (touch, counts), int32 tensors on the batch's device,
        or (touch, counts, pairs) when a pair list is asked for.  touch [n_scenes, max_particles, 4] at particle DATA indices
        (CONTACT_TOUCH_FIELDS names the columns): particles touching i, those of them whose label differs from i's (-1 without
        labels), the wall bits (WALL_LEFT x <= r, WALL_RIGHT x >= bounds - r, WALL_LOW y <= r, WALL_HIGH y >= bounds - r), the
        smallest data index touching i (-1: none); a row where no particle lives is (0, 0 or -1, 0, -1).  counts [n_scenes, 4]
        (CONTACT_COUNT_FIELDS): touching pairs (the true number, however short the list), pairs of different labels (-1 without
        labels), particles on a wall, particles touching another.  pairs [n_scenes, n, 2]: the pairs (i, j), i < j, in ascending
        order of (i, j), the first n of them, (-1, -1) behind the last; with other_body=True only pairs of different labels.
        labels: None, True (self.bodies() is called first and its labels are used), or an int32 tensor / device pointer of
        [n_scenes, max_particles] labels of the caller's own, which are only compared with each other.  pairs: 0 / None = no
        list, n = a new tensor of n pairs per scene, or a contiguous int32 tensor [n_scenes, n, 2] to write into.  touch /
        counts: a device pointer (int) or a contiguous int32 torch tensor of at least that many elements to write into.  Every
        word is written.  Only reads the batch, only enqueues; torch's current stream is ordered after it."""
        import torch
        n, maxp = self.n_scenes, self.max_particles
        max_pairs = 0
        if isinstance(pairs, torch.Tensor):
            self._device_buffer("contacts: pairs", pairs, "int32", n * 2 * 4)
            max_pairs = pairs.shape[1] if pairs.dim() == 3 and tuple(pairs.shape[::2]) == (n, 2) else pairs.numel() // (2 * n)
        elif pairs is not None:
            if isinstance(pairs, bool) or not isinstance(pairs, (int, np.integer)) or not 0 <= pairs < 2 ** 32:
                raise ValueError("contacts: pairs is a number of pairs per scene or an int32 torch tensor, not %r" % (pairs,))
            max_pairs = int(pairs)
        outs, ptrs, tensors = self._bind("contacts", [
            ("touch", touch, True, (n, maxp, CONTACT_WORDS), "int32"),
            ("pairs", pairs if isinstance(pairs, torch.Tensor) else None, max_pairs > 0, (n, max_pairs, 2), "int32"),
            ("counts", counts, True, (n, CONTACT_WORDS), "int32"),
            ("labels", (lambda: self.bodies()[0]) if labels is True else labels, labels is not None, (n, maxp), "int32")])
        vp = ctypes.c_void_p
        flags = CONTACTS_OTHER_BODY if other_body else 0
        self._ordered(tensors, lambda: load_library().sb_batch_contacts_device(self._h, flags, vp(ptrs[3]), vp(ptrs[0]), vp(ptrs[1]), max_pairs,
                                                                               vp(ptrs[2])))
        return (outs[0], outs[2], outs[1]) if max_pairs > 0 else (outs[0], outs[2])

    # ---- the beam graph (sb_batch_graph_device)
    def graph(self, ends=True, material=False, adjacency=False, skip_pending=False, counts=None):
        """Which particles every beam joins, with what material, and who hangs on whom, in every scene in one launch: the beam
        half of a graph network's edge list (contacts(pairs=n) is the contact half).  Nodes are the particles at particle DATA
        indices (the rows of state_tensors() and contacts()), edges the LISTED beams at beam DATA indices: the live beams, by
        bodies()' rule -- a pending break flag still connects -- or, with skip_pending=True, the live beams without a pending
        flag: what the next delete pass will leave.  Returns a Graph named tuple of tensors on the batch's device (None where
        not asked for), int32 unless said:
        ends [n_scenes, max_beams, 2]: at beam data index d the particle data indices {a, b} of the beam's record, (-1, -1) where
        d is not a listed beam; row d lines up with row d of state_tensors()'s beams.
        material [n_scenes, max_beams, 5] float32 (GRAPH_MATERIAL_FIELDS): length, spring, damp, yield_strain,
        strain_break_limit, verbatim bits; zeros where d is not listed.
        row_ptr [n_scenes, max_particles + 1] and nbr [n_scenes, 2 * max_beams, 2] (adjacency=True), a CSR adjacency: the rows
        row_ptr[p] .. row_ptr[p + 1] - 1 of nbr are {other endpoint, beam data index} of the listed beams at particle p, in
        ascending order of beam data index; (-1, -1) behind the last.  The same bits on every run.
        counts [n_scenes, 4] (GRAPH_COUNT_FIELDS): listed beams, particles of degree >= 1, the largest degree, the smallest data
        index of a particle of that degree (-1: no beam listed).  counts=None: made whenever something else is; False: not.
        A scene never uploaded gives -1 / 0 rows.  ends / material / counts: True, False, a device pointer (int) or a contiguous
        torch tensor to write into; adjacency: True, False or a pair (row_ptr, nbr) of those.  Every word of what is asked for
        is written.  Only reads the batch, only enqueues; torch's current stream is ordered after it."""
        n, maxp, maxb = self.n_scenes, self.max_particles, self.max_beams
        if isinstance(adjacency, (tuple, list)):
            if len(adjacency) != 2:
                raise ValueError("graph: adjacency is True, False or a pair (row_ptr, nbr)")
            row_ptr, nbr = adjacency
        else:
            row_ptr = nbr = bool(adjacency)
        if nbr is not False and nbr is not None and (row_ptr is False or row_ptr is None):
            raise ValueError("graph: nbr without row_ptr")
        if counts is None:
            counts = True
        wanted = [x is not False and x is not None for x in (ends, material, row_ptr, nbr, counts)]
        given = [None if isinstance(x, bool) else x for x in (ends, material, row_ptr, nbr, counts)]   # (True: a new tensor)
        outs, ptrs, tensors = self._bind("graph", [("ends", given[0], wanted[0], (n, maxb, 2), "int32"),
                                                   ("material", given[1], wanted[1], (n, maxb, GRAPH_MATERIAL_WORDS), "float32"),
                                                   ("row_ptr", given[2], wanted[2], (n, maxp + 1), "int32"),
                                                   ("nbr", given[3], wanted[3], (n, 2 * maxb, 2), "int32"),
                                                   ("counts", given[4], wanted[4], (n, GRAPH_COUNT_WORDS), "int32")])
        vp = ctypes.c_void_p
        self._ordered(tensors, lambda: load_library().sb_batch_graph_device(self._h, GRAPH_SKIP_PENDING if skip_pending else 0,
                                                                            *[vp(p) for p in ptrs]))
        return Graph(*outs)

    # ---- what the two queries share (csrc/sb_batch_query.h)
    def _query(self, call, items, result, rows, labels, rest, outs):
        """raycast() and nearest() behind their output lists: `rows` is [n_scenes, k, 8], an int32 / float32 torch tensor or
        (device pointer, k), `items` its name in the errors.  outs: (name, what the caller passed, shape after [n_scenes, k],
        dtype) in the C call's order, the counts last (shape None: [n_scenes, 4]); the first two are never None, a None among the
        others means `rest`, or with rest=None "whenever one of the first two is made".  Binds the outputs and the labels
        (labels=True: bodies()'s), zeroes the counts of k == 0, makes the ordered call sb_batch_<call>_device and returns
        result(*outputs)."""
        import torch
        n, k_max = self.n_scenes, RAY_MAX   # (NEAR_MAX, NEAR_ROW_WORDS and NEAR_COUNT_WORDS are the same numbers: one plan)
        if isinstance(rows, tuple):
            rptr, k, is_tensor = int(rows[0]), int(rows[1]), False
        else:
            if not isinstance(rows, torch.Tensor) or rows.dtype not in (torch.int32, torch.float32):
                raise ValueError("%s: %s must be an int32 / float32 torch tensor [n_scenes, k, 8] or (device pointer, k)" % (call, items))
            if rows.dim() != 3 or rows.shape[0] != n or rows.shape[2] != RAY_ROW_WORDS or rows.shape[1] > k_max:
                raise ValueError("%s: %s must be [n_scenes = %d, k <= %d, 8], not %s" % (call, items, n, k_max, tuple(rows.shape)))
            k = int(rows.shape[1])
            rptr, is_tensor = self._device_buffer("%s: %s" % (call, items), rows, None, n * k * RAY_ROW_WORDS * 4)
        if not 0 <= k <= k_max:
            raise ValueError("%s: k is %d, not in 0 .. %d" % (call, k, k_max))
        asked = [x for _, x, _, _ in outs]
        if rest is None:
            rest = any(x is not False and x is not None for x in asked[:2])
        asked = asked[:2] + [rest if x is None else x for x in asked[2:]]
        wanted = [x is not False and x is not None for x in asked]
        names = [name for name, _, _, _ in outs]
        if not any(wanted):
            raise ValueError("%s: %s and %s are all False: nothing to write" % (call, ", ".join(names[:-1]), names[-1]))
        bufs, ptrs, tensors = self._bind(call, [
            (name, None if isinstance(x, bool) else x, w, (n, RAY_COUNT_WORDS) if tail is None else (n, k) + tail, dtype)   # (True: a new tensor)
            for (name, _, tail, dtype), x, w in zip(outs, asked, wanted)] + [
            ("labels", (lambda: self.bodies()[0]) if labels is True else labels, labels is not None, (n, self.max_particles), "int32")])
        if k == 0:   # (the library enqueues nothing for no rows: the counts of no rows are zeros)
            if isinstance(bufs[-2], torch.Tensor):
                bufs[-2].zero_()
            return result(*bufs[:-1])
        vp = ctypes.c_void_p
        fn = getattr(load_library(), "sb_batch_%s_device" % call)
        self._ordered(tensors or is_tensor, lambda: fn(self._h, 0, vp(rptr), k, vp(ptrs[-1]), *[vp(p) for p in ptrs[:-1]]))
        return result(*bufs[:-1])

    # ---- range sensors (sb_batch_raycast_device)
    def raycast(self, rays, labels=None, t=True, hit=True, counts=None):
        """"How far is the nearest thing in this direction, and what is it?": every scene casts its own k rays in one launch.
        `rays` is [n_scenes, k, 8], k <= RAY_MAX, in sb_batch_ray's layout {mask, ox, oy, dx, dy, tmax, skip_label, 0} -- mask and
        skip_label integers, the five floats as their bits: an int32 or float32 (bits) torch tensor on the batch's device
        (ray_rows() packs one), or a tuple (device pointer, k).  A ray is origin + t * direction for 0 <= t <= tmax; it meets the
        scene's particles as discs of the batch's particle_radius (RAY_PARTICLES), its live beams as segments (RAY_BEAMS; a
        pending break flag still counts, as for bodies()) and the four walls (RAY_WALLS); include/softbody.h states every test.
        The nearest meeting wins; on equal t a particle beats a beam beats a wall, then the smaller index.  Returns a RayCast
        named tuple of tensors on the batch's device (None where not asked for):
        t [n_scenes, k] float32: the hit's t (a distance when the direction is a unit vector), the row's tmax on a miss, 0 for
        an empty (mask 0) or invalid row.
        hit [n_scenes, k, 3] int32 (RAY_HIT_FIELDS): kind (RAY_MISS, RAY_PARTICLE, RAY_BEAM, RAY_WALL, RAY_EMPTY, RAY_INVALID),
        index (the particle's or beam's DATA index, the WALL_* word, -1 where nothing was hit), label (of the hit particle or of
        the hit beam's endpoint a; -1 for walls, misses and without labels).
        counts [n_scenes, 4] int32 (RAY_COUNT_FIELDS): valid rows, hits on particles, on beams, on walls.  counts=None: made
        whenever something else is; False: not.
        labels: None, True (self.bodies() is called first, on the same stream, and its labels are used), or an int32 tensor /
        device pointer of [n_scenes, max_particles] labels of the caller's own at particle data indices, which are only compared:
        a row whose skip_label is not -1 ignores the particles of that label and the beams whose endpoint a carries it, so a
        sensor that rides on a body sees past it.  t / hit / counts: True, False, a device pointer (int) or a contiguous torch
        tensor to write into.  Every word of what is asked for is written, the same bits on every run (k == 0: counts are
        zeros).  Only reads the batch, only enqueues; torch's current stream is ordered after it."""
        return self._query("raycast", "rays", RayCast, rays, labels, True,
                           [("t", t, (), "float32"), ("hit", hit, (RAY_HIT_WORDS,), "int32"), ("counts", counts, None, "int32")])

    # ---- proximity queries (sb_batch_nearest_device)
    def nearest(self, points, labels=None, d=True, hit=True, point=None, within=None, counts=None):
        """"What is nearest to this point, how far is it, and how much is within reach?": every scene asks about its own k points
        in one launch.  `points` is [n_scenes, k, 8], k <= NEAR_MAX, in sb_batch_near_point's layout {mask, px, py, rmax,
        skip_label, 0, 0, 0} -- mask and skip_label integers, the three floats as their bits: an int32 or float32 (bits) torch
        tensor on the batch's device (point_rows() packs one), or a tuple (device pointer, k).  A point is measured against the
        scene's particles (their centres, NEAR_PARTICLES), its live beams as segments (NEAR_BEAMS; a pending break flag still
        counts, as for bodies()) and the four walls (NEAR_WALLS); whatever lies farther than rmax is not kept;
        include/softbody.h states every expression.  The nearest kept wins; on equal distance a particle beats a beam beats a
        wall, then the smaller index.  Returns a Nearest named tuple of tensors on the batch's device (None where not asked for):
        d [n_scenes, k] float32: the distance to the winner, the row's rmax on a miss, 0 for an empty (mask 0) or invalid row.
        hit [n_scenes, k, 3] int32 (NEAR_HIT_FIELDS): kind (NEAR_MISS, NEAR_PARTICLE, NEAR_BEAM, NEAR_WALL, NEAR_EMPTY,
        NEAR_INVALID), index (the particle's or beam's DATA index, the WALL_* word, -1 where there is no winner), label (of the
        winning particle or of the winning beam's endpoint a; -1 for walls, misses and without labels).
        point [n_scenes, k, 2] float32: the closest point on the winner -- where a grab attaches; the query point on a miss.
        within [n_scenes, k, 2] int32 (NEAR_WITHIN_FIELDS): how many particles and how many live beams lie within rmax (0 for a
        class the mask leaves out).
        counts [n_scenes, 4] int32 (NEAR_COUNT_FIELDS): valid rows, rows whose nearest is a particle, a beam, a wall.
        point / within / counts = None: made whenever d or hit is; False: not.
        labels: None, True (self.bodies() is called first, on the same stream, and its labels are used), or an int32 tensor /
        device pointer of [n_scenes, max_particles] labels of the caller's own at particle data indices, which are only compared:
        a row whose skip_label is not -1 ignores the particles of that label and the beams whose endpoint a carries it.
        d / hit / point / within / counts: True, False, a device pointer (int) or a contiguous torch tensor to write into.  Every
        word of what is asked for is written, the same bits on every run (k == 0: counts are zeros).  Only reads the batch, only
        enqueues; torch's current stream is ordered after it.

        Grasping -- weld each scene's hand particle (data index `hand` [n_scenes]) to whatever particle is within reach:
            near = be.nearest(point_rows(hand_pos[:, None, :], reach, mask=NEAR_PARTICLES, skip_label=hand_label[:, None]), labels=True)
            partner = torch.where(near.hit[..., 0] == NEAR_PARTICLE, near.hit[..., 1], -1)
            pairs = torch.stack((partner, hand[:, None].expand_as(partner)), -1)
            be.add_beams(new_beam_rows(pairs, spring, damp, yield_strain, strain_break_limit), length_current=True, skip_joined=True)
        A row whose partner is -1 is an empty row of add_beams (ADD_EMPTY); nothing is read back."""
        return self._query("nearest", "points", Nearest, points, labels, None,
                           [("d", d, (), "float32"), ("hit", hit, (NEAR_HIT_WORDS,), "int32"), ("point", point, (2,), "float32"),
                            ("within", within, (2,), "int32"), ("counts", counts, None, "int32")])

    # ---- beam and contact forces per particle (sb_batch_forces_device)
    def forces(self, labels=None, other_body=False, rows=True, beam_i32=None, tension=None, counts=None):
        """How hard every beam pulls and every contact pushes, in every scene in one launch: the forces the NEXT substep would
        compute from the CURRENT state, in the step's own arithmetic, bit for bit (include/softbody.h states the definition).
        Nothing is applied: no yield, no last_length update, no break flag, no particle moved.  Returns a Forces named tuple of
        tensors on the batch's device (None where not asked for):
        rows [n_scenes, max_particles, 8] float32 at particle DATA indices (FORCE_FIELDS names the columns): beam_x, beam_y, the
        sum of the beam forces on the particle (the fixed-point sum times 2^-16, what the integration adds to the acceleration);
        push_x, push_y, what the contacts add to the acceleration; impulse_x, impulse_y, what they add to the velocity; depth, the
        largest overlap 2r - dist among the partners; partners, their number.  Eight zeros where no particle lives.
        beam_i32 [n_scenes, max_particles, 2] int32: the fixed-point beam force sums themselves (wrapping, saturating).
        tension [n_scenes, max_beams] float32 at beam DATA indices: the beam's force_mag, the reference's sign: positive when the beam
        is compressed and pushes its endpoints apart, negative when it is stretched and pulls; 0 where no live beam is.  A beam with a pending break flag still pulls.
        counts [n_scenes, 4] int32 (FORCE_COUNT_FIELDS): particles, beams evaluated, particles with a partner, beams whose
        tension is not finite.
        labels: None, True (self.bodies() is called first, on the same stream, and its labels are used), or an int32 tensor /
        device pointer of [n_scenes, max_particles] labels of the caller's own; with other_body=True only partners whose label
        differs from the particle's are taken: what another body does to this one.  rows / beam_i32 / tension / counts: True (a
        new tensor), None / False (not wanted), a device pointer (int) or a contiguous torch tensor to write into; every word of
        what is asked for is written.  Only reads the batch, only enqueues; torch's current stream is ordered after it.
        Grip force on body L, per scene -- the contacts' push on its particles from everybody else, summed:
            f = be.forces(labels=True, other_body=True)
            labels = be.bodies()[0]                                        # [n, max_particles], -1 where no particle lives
            grip = torch.zeros(n, max_particles, 2, device=f.rows.device)
            flat = (labels + max_particles * torch.arange(n, device=labels.device)[:, None]).clamp_min(0).view(-1)
            grip.view(-1, 2).index_add_(0, flat.long(), f.rows[..., 2:4].reshape(-1, 2))   # (rows of no particle add zeros)
            grip[s, L] is then the push on the body labelled L of scene s.
        Muscle force -- the force the beams of a muscle carry, at the rows of state_tensors()'s beams:
            tension = be.forces(rows=None, tension=True).tension           # [n, max_beams], row d == row d of state_tensors()[1]
            muscle_force = tension[:, muscle_beam_indices]"""
        n, maxp, maxb = self.n_scenes, self.max_particles, self.max_beams
        wanted = [x is not False and x is not None for x in (rows, beam_i32, tension, counts)]
        given = [None if isinstance(x, bool) else x for x in (rows, beam_i32, tension, counts)]   # (True: a new tensor)
        outs, ptrs, tensors = self._bind("forces", [
            ("rows", given[0], wanted[0], (n, maxp, FORCE_WORDS), "float32"),
            ("beam_i32", given[1], wanted[1], (n, maxp, 2), "int32"),
            ("tension", given[2], wanted[2], (n, maxb), "float32"),
            ("counts", given[3], wanted[3], (n, len(FORCE_COUNT_FIELDS)), "int32"),
            ("labels", (lambda: self.bodies()[0]) if labels is True else labels, labels is not None, (n, maxp), "int32")])
        vp = ctypes.c_void_p
        flags = FORCES_OTHER_BODY if other_body else 0
        self._ordered(tensors, lambda: load_library().sb_batch_forces_device(self._h, flags, vp(ptrs[4]), *[vp(p) for p in ptrs[:4]]))
        return Forces(*outs[:4])

    # ---- pictures (sb_batch_render_device / sb_batch_render_scene)
    def _render_options(self, resolution, bounds_size, particle_radius, first=0, count=0):
        o = SbBatchRenderOptions()
        o.struct_size = ctypes.sizeof(SbBatchRenderOptions)
        o.resolution = int(resolution)
        o.bounds_size = 0.0 if bounds_size is None else float(bounds_size)
        o.particle_radius = 0.0 if particle_radius is None else float(particle_radius)
        o.first, o.count = first, count
        return o

    def render(self, resolution=64, bounds_size=None, particle_radius=None, first=0, count=None, out=None):
        """One picture per scene first .. first+count-1 (count=None: every scene from `first` on), all drawn in one launch: a
        torch.uint8 tensor [count, resolution, resolution, 3] on the batch's device, each picture host/render.js's renderPPM
        body (RGB8, rows top to bottom) of what load_scene would return now; scenes never uploaded or empty are black.
        None = the batch's own bounds / radius.  `out`: a device pointer (int) or a contiguous uint8 torch tensor of at least
        count * resolution^2 * 3 bytes to draw into.  Only enqueues; torch's current stream is ordered after the render."""
        res = int(resolution)
        if not 0 < res <= BATCH_RENDER_MAX_RESOLUTION:
            raise ValueError("render: resolution %d is not in 1 .. %d" % (res, BATCH_RENDER_MAX_RESOLUTION))
        first = int(first)
        count = self.n_scenes - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > self.n_scenes:
            raise ValueError("render: scenes %d .. %d+%d are not all inside the batch of %d" % (first, first, count, self.n_scenes))
        (out,), (ptr,), t = self._bind("render", [("out", out, True, (count, res, res, 3), "uint8")])
        o = self._render_options(res, bounds_size, particle_radius, first, count)
        self._ordered(t, lambda: load_library().sb_batch_render_device(self._h, ctypes.byref(o), ctypes.c_void_p(ptr)))
        return out

    def render_scene(self, i, resolution=64, bounds_size=None, particle_radius=None):
        """Scene i's picture as a numpy (resolution, resolution, 3) uint8 array.  Waits for the stream."""
        res = int(resolution)
        if not 0 < res <= BATCH_RENDER_MAX_RESOLUTION:
            raise ValueError("render_scene: resolution %d is not in 1 .. %d" % (res, BATCH_RENDER_MAX_RESOLUTION))
        out = np.empty((res, res, 3), dtype=np.uint8)
        o = self._render_options(res, bounds_size, particle_radius)
        self._check(load_library().sb_batch_render_scene(self._h, int(i), ctypes.byref(o), _ptr(out), out.nbytes))
        return out
