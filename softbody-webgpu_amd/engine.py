"""ctypes binding of the C ABI in include/softbody.h (libsoftbody_hip.so).

The HIP library is the product; this module only marshals numpy buffers into it.  There is
no CPU fallback: if the library is missing, lacks a declared symbol, or finds no GPU, the
calls raise.
"""
import collections
import ctypes
import os
import re

import numpy as np

from .device_binding import DeviceBinding
from .layout import BEAM_STRIDE, LAYOUT_V1, METADATA_BYTES, PARTICLE_STRIDE, Buffers

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SOFTBODY_HIP_LIB") or os.path.join(_HERE, "csrc", "libsoftbody_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "softbody.h")

COLLIDE_OFF, COLLIDE_ALLPAIRS, COLLIDE_GRID = 0, 1, 2
PATH_AUTO, PATH_ATOMIC, PATH_TILED = 0, 1, 2

STATUS = {0: "SB_OK", 1: "SB_ERR_INVALID", 2: "SB_ERR_HIP", 3: "SB_ERR_NO_DEVICE", 4: "SB_ERR_OOM",
          5: "SB_ERR_STATE", 6: "SB_ERR_UNSUPPORTED"}


class EngineError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s: %s" % (STATUS.get(status, status), message))
        self.status = status


class SbOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("bounds_size", ctypes.c_float),
                ("particle_radius", ctypes.c_float), ("subticks", ctypes.c_uint32),
                ("max_particles", ctypes.c_uint32), ("max_beams", ctypes.c_uint32),
                ("layout", ctypes.c_uint32), ("collision_mode", ctypes.c_uint32),
                ("path", ctypes.c_uint32), ("tile_particles", ctypes.c_uint32),
                ("device_ordinal", ctypes.c_int32), ("grid_skin", ctypes.c_float),
                ("block_substeps", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class SbSummaryOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("partials", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 6)]


SUMMARY_WORDS = 24           # SB_SUMMARY_WORDS
SUMMARY_COUNT_WORDS = 8      # the uint64 counts beside the row
# the counts, in order (include/softbody.h, sb_summary_device); the row's words are batch.SUMMARY_FIELDS (engine.SUMMARY_FIELDS)
SUMMARY_COUNT_FIELDS = ("particles", "live_beams", "removed_beams", "pending_breaks", "nonfinite_particles", "nonfinite_beams",
                        "uploaded", "reserved_7")


class SbGraphOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("max_half_edges", ctypes.c_uint64),
                ("reserved", ctypes.c_uint32 * 4)]


GRAPH_SKIP_PENDING = 1                                # SB_GRAPH_SKIP_PENDING
GRAPH_COUNT_WORDS = 4                                 # SB_GRAPH_COUNT_WORDS
# the words of graph()'s counts, in order (include/softbody.h, sb_graph_device)
GRAPH_COUNT_FIELDS = ("beams", "connected_particles", "max_degree", "max_degree_particle")


class SbRaycastOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("cells_per_side", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 5)]


RAYCAST_COUNT_WORDS = 8                               # SB_RAYCAST_COUNT_WORDS
RAYCAST_MAX_RAYS = 1 << 24                            # rows of one call
# the words of raycast()'s counts, in order (include/softbody.h, sb_raycast_device): four of the definition, three of the cost
RAYCAST_COUNT_FIELDS = ("valid", "particles", "beams", "walls", "swept_rows", "particles_outside_grid", "long_beams", "reserved_7")
RayCast = collections.namedtuple("RayCast", ("t", "hit", "counts"))


def ray_rows(origin, direction, tmax, mask=7, skip_label=None):
    """Rows for Engine.raycast() from a float32 torch tensor [n, 2] of origins: batch.ray_rows() on one scene of n rows, an int32
    tensor [n, 8] in sb_batch_ray's layout.  direction, tmax, mask, skip_label: as there, broadcasting to [n, 2] / [n]."""
    import torch
    from . import batch
    if not isinstance(origin, torch.Tensor) or origin.dim() != 2:
        raise ValueError("ray_rows: origin must be a float32 torch tensor [n, 2]")
    return batch.ray_rows(origin[None], direction, tmax, mask=mask, skip_label=skip_label)[0]


class SbNearestOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("cells_per_side", ctypes.c_uint32),
                ("max_rings", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 4)]


NEAREST_COUNT_WORDS = 8                               # SB_NEAREST_COUNT_WORDS
NEAREST_MAX_POINTS = 1 << 24                          # rows of one call
# the words of nearest()'s counts, in order (include/softbody.h, sb_nearest_device): four of the definition, three of the cost
NEAREST_COUNT_FIELDS = ("valid", "particles", "beams", "walls", "swept_rows", "particles_outside_grid", "long_beams", "reserved_7")
Nearest = collections.namedtuple("Nearest", ("d", "hit", "point", "within", "counts"))


class SbBodiesOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 7)]


BODY_WORDS = 4               # SB_BODY_WORDS: the int64 counts of bodies(); batch.BODY_FIELDS (engine.BODY_FIELDS) names them


class SbContactsOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("max_pairs", ctypes.c_uint64),
                ("reserved", ctypes.c_uint32 * 4)]


CONTACT_WORDS = 4            # SB_CONTACT_WORDS: the int32 words of a touch row; batch.CONTACT_TOUCH_FIELDS names them
CONTACT_COUNT_WORDS = 4      # SB_CONTACT_COUNT_WORDS: the int64 counts of contacts(); batch.CONTACT_COUNT_FIELDS names them
CONTACTS_OTHER_BODY = 1      # SB_CONTACTS_OTHER_BODY


class SbForcesOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 6)]


FORCE_WORDS = 8              # SB_FORCE_WORDS: the floats of a row of forces(); batch.FORCE_FIELDS names them
FORCE_COUNT_WORDS = 4        # SB_FORCE_COUNT_WORDS: the int64 counts of forces(); batch.FORCE_COUNT_FIELDS names them
FORCES_OTHER_BODY = 1        # SB_FORCES_OTHER_BODY


class SbBodySummaryOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 5), ("max_rows", ctypes.c_uint64)]


BODY_SUMMARY_WORDS = 24          # SB_BODY_SUMMARY_WORDS: the floats of a row of body_summary(); batch.BODY_SUMMARY_FIELDS names them
BODY_SUMMARY_COUNT_WORDS = 8     # SB_BODY_SUMMARY_COUNT_WORDS: the exact int64 words beside a row
# the int64 words of a row of body_summary()'s counts, in order (include/softbody.h, sb_body_summary_device)
BODY_SUMMARY_COUNT_FIELDS = ("particles", "live_beams", "label", "pending_breaks", "nonfinite_particles", "nonfinite_beams",
                             "finite_particles", "reserved_7")


class SbCutOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 6)]


CUT_NONE, CUT_SEGMENT, CUT_DISC = 0, 1, 2     # SB_CUT_*: the kind word of a shape
CUT_MAX_SHAPES = 64                           # SB_CUT_MAX_SHAPES
CUT_SHAPE_WORDS = 8                           # a shape: {kind, x0, y0, x1, y1, 0, 0, 0}
CUT_DRY_RUN = 1                               # SB_CUT_DRY_RUN
CUT_COUNT_FIELDS = ("tested", "hit", "flagged", "already_flagged")   # the counts of cut(), in order (SB_CUT_COUNT_WORDS of them)


def cut_shapes(segments=(), discs=()):
    """Rows of shapes for Engine.cut() / BatchEngine.cut(): segments (x0, y0, x1, y1) -- a knife from (x0, y0) to (x1, y1) --
    then discs (x, y, r) -- an eraser at (x, y) of radius r -- as a uint32 numpy array [n, 8] in sb_cut_shape's layout (the kind
    as an integer word, the coordinates as float32 bits)."""
    seg = np.asarray(segments, dtype=np.float32).reshape(-1, 4)
    dsc = np.asarray(discs, dtype=np.float32).reshape(-1, 3)
    rows = np.zeros((len(seg) + len(dsc), CUT_SHAPE_WORDS), dtype=np.uint32)
    rows[:len(seg), 0] = CUT_SEGMENT
    rows[:len(seg), 1:5] = seg.view(np.uint32)
    rows[len(seg):, 0] = CUT_DISC
    rows[len(seg):, 1:4] = dsc.view(np.uint32)
    return rows


def host_shapes(shapes, ndim=2):
    """`shapes` as a uint32 numpy array [..., 8] in sb_cut_shape's layout.  An int32 / uint32 array is taken as the words
    themselves (cut_shapes() makes one); any other array or a nested list holds numbers (the kind too), in rows of 5
    (kind, x0, y0, x1, y1) or 8."""
    a = np.asarray(shapes)
    if a.size == 0:
        a = a.reshape((0,) * (ndim - 1) + (CUT_SHAPE_WORDS,)) if a.ndim < ndim else a
    if a.ndim != ndim or a.shape[-1] not in (5, CUT_SHAPE_WORDS):
        raise ValueError("cut: shapes must be %d-dimensional with rows of 5 or 8 words, not %s" % (ndim, a.shape))
    if a.dtype in (np.dtype(np.int32), np.dtype(np.uint32)):
        w = np.ascontiguousarray(a).view(np.uint32)
    else:
        f = a.astype(np.float32)
        kind = f[..., 0]
        if not np.all(np.isin(kind, (CUT_NONE, CUT_SEGMENT, CUT_DISC))):
            raise ValueError("cut: a shape's kind must be CUT_NONE, CUT_SEGMENT or CUT_DISC")
        w = np.ascontiguousarray(f).view(np.uint32).copy()
        w[..., 0] = kind.astype(np.uint32)
    out = np.zeros(w.shape[:-1] + (CUT_SHAPE_WORDS,), dtype=np.uint32)
    out[..., :w.shape[-1]] = w
    return out


def device_shapes(shapes, dev, ndim=2):
    """`shapes` as a contiguous int32 torch tensor [..., 8] on `dev` in sb_cut_shape's layout: an int32 tensor as it is, a float32
    tensor with its kind column converted on the device, anything else through host_shapes()."""
    import torch
    if isinstance(shapes, torch.Tensor):
        if shapes.dim() != ndim or shapes.shape[-1] != CUT_SHAPE_WORDS or shapes.dtype not in (torch.int32, torch.float32):
            raise ValueError("cut: a tensor of shapes must be float32 / int32 with %d dimensions and rows of 8 words" % ndim)
        if shapes.device != dev and not (shapes.device.type == dev.type and shapes.device.index in (None, dev.index)):
            raise ValueError("cut: the shapes are on %s, not on %s" % (shapes.device, dev))
        if shapes.dtype == torch.int32:
            return shapes.contiguous()
        words = shapes.contiguous().view(torch.int32).clone()
        words[..., 0] = shapes[..., 0].to(torch.int32)
        return words
    return torch.from_numpy(host_shapes(shapes, ndim).view(np.int32)).to(dev)


def __getattr__(name):
    if name in ("SUMMARY_FIELDS", "BODY_FIELDS", "BODY_SUMMARY_FIELDS", "CONTACT_TOUCH_FIELDS", "CONTACT_COUNT_FIELDS", "FORCE_FIELDS", "FORCE_COUNT_FIELDS", "Forces", "WALL_LEFT", "WALL_RIGHT", "WALL_LOW",
                "WALL_HIGH"):  # the batch's words: its names are not copied (batch.py imports this module)
        from . import batch
        return getattr(batch, name)
    raise AttributeError(name)


class SbRenderOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("resolution", ctypes.c_uint32), ("bounds_size", ctypes.c_double),
                ("particle_radius", ctypes.c_double), ("reserved", ctypes.c_uint32 * 4)]


RENDER_MAX_RESOLUTION = 16384
BEAM_TARGET_LENGTH, BEAM_LAST_LENGTH = 1, 2          # SB_BEAM_* (sb_write_beams_device)

GUARD_SLAB, GUARD_BAND, GUARD_BEAM, GUARD_MOTION = 1, 2, 4, 8     # SB_GUARD_* (include/softbody.h sb_halo_guard)
GUARD_KIND_NAMES = {GUARD_SLAB: "A", GUARD_BAND: "B", GUARD_BEAM: "C", GUARD_MOTION: "D"}


class SbHaloGuardDesc(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("rank", ctypes.c_uint32), ("world", ctypes.c_uint32),
                ("depth", ctypes.c_uint32), ("contact_reach", ctypes.c_float), ("hop", ctypes.c_float),
                ("motion", ctypes.c_float), ("n_own_particles", ctypes.c_uint32), ("own_particles", ctypes.c_void_p),
                ("held", ctypes.c_void_p), ("n_own_beams", ctypes.c_uint32), ("own_beams", ctypes.c_void_p),
                ("lo", ctypes.c_void_p), ("hi", ctypes.c_void_p), ("reserved", ctypes.c_uint32 * 4)]


class SbHaloGuardReport(ctypes.Structure):
    _fields_ = [("kinds", ctypes.c_uint32), ("violations", ctypes.c_uint32), ("refreshes", ctypes.c_uint32),
                ("first_refresh", ctypes.c_uint32), ("first_is_beam", ctypes.c_uint32), ("first_index", ctypes.c_uint32),
                ("motion", ctypes.c_float), ("reserved", ctypes.c_uint32)]


class GuardStatus:
    """sb_halo_guard_report: the verdict of an engine's halo guard.  `kinds` = SB_GUARD_* bits (0: nothing fired);
    `first_refresh` / `first_is_beam` / `first_index` (LOCAL data index) name the first offending item, or are None."""

    def __init__(self, r):
        self.kinds, self.violations, self.refreshes, self.motion = r.kinds, r.violations, r.refreshes, r.motion
        fired = r.first_refresh != 0xFFFFFFFF
        self.first_refresh = r.first_refresh if fired else None
        self.first_is_beam = bool(r.first_is_beam) if fired else None
        self.first_index = r.first_index if fired else None

    @property
    def kind_names(self):
        return "".join(n for bit, n in sorted(GUARD_KIND_NAMES.items()) if self.kinds & bit)

    def __repr__(self):
        return ("GuardStatus(kinds=%r, violations=%d, refreshes=%d, first_refresh=%r, first_is_beam=%r, first_index=%r)"
                % (self.kind_names, self.violations, self.refreshes, self.first_refresh, self.first_is_beam, self.first_index))

_lib = None


def declared_symbols():
    """Every function include/softbody.h declares."""
    src = open(HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sb_[a-z_0-9]+)\s*\(", src)))


def load_library():
    """dlopen the HIP engine and check it exports every symbol the header declares."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)" % LIB_PATH)
    # One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so.7 /
    # libhsa-runtime64.so.1 and load them by path; if this library pulled in /opt/rocm's copies
    # first, a later `import torch` would bring up a SECOND runtime in the process, whose device
    # discovery fails ("No HIP GPUs are available").  Loading torch's copy first makes our
    # DT_NEEDED libamdhip64.so.7 resolve to the already-loaded one, so torch (RCCL, streams) and the
    # engine share a single runtime and can share hipStream_t handles (halo.TorchTransport).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    missing = [s for s in declared_symbols() if not hasattr(L, s)]
    if missing:
        raise ImportError("libsoftbody_hip.so lacks symbols declared in softbody.h: %s" % missing)
    vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    L.sb_default_options.argtypes = [ctypes.POINTER(SbOptions)]
    L.sb_default_options.restype = None
    L.sb_create.argtypes = [ctypes.POINTER(SbOptions), ctypes.POINTER(vp)]
    L.sb_destroy.argtypes = [vp]
    L.sb_write_buffers.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, sz]
    L.sb_load_buffers.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, sz]
    L.sb_write_user_input.argtypes = [vp, vp]
    L.sb_set_physics_constants.argtypes = [vp, vp]
    L.sb_get_physics_constants.argtypes = [vp, vp]
    L.sb_frame.argtypes = [vp]
    L.sb_step.argtypes = [vp, u32]
    L.sb_delete_pass.argtypes = [vp]
    L.sb_halo_delete_ghosts.argtypes = [vp]
    L.sb_sync.argtypes = [vp]
    L.sb_step_timed.argtypes = [vp, u32, ctypes.POINTER(ctypes.c_float)]
    L.sb_mark.argtypes = [vp, u32]
    L.sb_mark_elapsed.argtypes = [vp, u32, u32, ctypes.POINTER(ctypes.c_float)]
    L.sb_get_counts.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.sb_get_info.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
    L.sb_halo_configure.argtypes = [vp, vp, u32, vp, u32, vp, u32, vp, u32]
    L.sb_halo_set_layout.argtypes = [vp, vp, vp, vp, vp]
    L.sb_halo_pack.argtypes = [vp, vp]
    L.sb_peer_mailbox.argtypes = [vp, ctypes.POINTER(vp), vp, ctypes.POINTER(ctypes.c_uint64)]
    L.sb_peer_map.argtypes = [vp, vp, ctypes.POINTER(vp)]
    L.sb_peer_connect.argtypes = [vp, u32, ctypes.POINTER(vp), vp, vp, vp, vp, vp, u32]
    L.sb_peer_exchange.argtypes = [vp]
    L.sb_halo_unpack.argtypes = [vp, vp]
    L.sb_halo_guard.argtypes = [vp, ctypes.POINTER(SbHaloGuardDesc)]
    L.sb_halo_guard_status.argtypes = [vp, ctypes.POINTER(SbHaloGuardReport)]
    L.sb_get_stream.argtypes = [vp, ctypes.POINTER(vp)]
    L.sb_render.argtypes = [vp, ctypes.POINTER(SbRenderOptions), vp, sz]
    L.sb_render_device.argtypes = [vp, ctypes.POINTER(SbRenderOptions), vp]
    L.sb_read_state_device.argtypes = [vp, vp, vp, vp]
    L.sb_write_particles_device.argtypes = [vp, vp]
    L.sb_write_beams_device.argtypes = [vp, vp, u32]
    L.sb_checkpoint_device.argtypes = [vp]
    L.sb_restore_device.argtypes = [vp]
    L.sb_cut_device.argtypes = [vp, ctypes.POINTER(SbCutOptions), vp, u32, vp, vp]
    L.sb_cut.argtypes = [vp, ctypes.POINTER(SbCutOptions), vp, u32, vp, vp]
    L.sb_summary_device.argtypes = [vp, ctypes.POINTER(SbSummaryOptions), vp, vp]
    L.sb_summary.argtypes = [vp, ctypes.POINTER(SbSummaryOptions), vp, vp]
    L.sb_graph_device.argtypes = [vp, ctypes.POINTER(SbGraphOptions), vp, vp, vp, vp]
    L.sb_graph.argtypes = [vp, ctypes.POINTER(SbGraphOptions), vp, vp, vp, vp]
    L.sb_raycast_device.argtypes = [vp, ctypes.POINTER(SbRaycastOptions), vp, u32, vp, vp, vp, vp]
    L.sb_raycast.argtypes = [vp, ctypes.POINTER(SbRaycastOptions), vp, u32, vp, vp, vp, vp]
    L.sb_nearest_device.argtypes = [vp, ctypes.POINTER(SbNearestOptions), vp, u32, vp, vp, vp, vp, vp, vp]
    L.sb_nearest.argtypes = [vp, ctypes.POINTER(SbNearestOptions), vp, u32, vp, vp, vp, vp, vp, vp]
    L.sb_bodies_device.argtypes = [vp, ctypes.POINTER(SbBodiesOptions), vp, vp, vp]
    L.sb_bodies.argtypes = [vp, ctypes.POINTER(SbBodiesOptions), vp, vp, vp]
    L.sb_contacts_device.argtypes = [vp, ctypes.POINTER(SbContactsOptions), vp, vp, vp, vp]
    L.sb_contacts.argtypes = [vp, ctypes.POINTER(SbContactsOptions), vp, vp, vp, vp]
    L.sb_forces_device.argtypes = [vp, ctypes.POINTER(SbForcesOptions), vp, vp, vp, vp, vp]
    L.sb_forces.argtypes = [vp, ctypes.POINTER(SbForcesOptions), vp, vp, vp, vp, vp]
    L.sb_body_summary_device.argtypes = [vp, ctypes.POINTER(SbBodySummaryOptions), vp, vp, vp, vp]
    L.sb_body_summary.argtypes = [vp, ctypes.POINTER(SbBodySummaryOptions), vp, vp, vp, vp]
    f32 = ctypes.c_float
    L.sb_partition_create.argtypes = [u32, u32, u32, vp, vp, vp, vp, u32, u32, f32, ctypes.POINTER(vp)]
    L.sb_partition_destroy.argtypes = [vp]
    L.sb_partition_rank_counts.argtypes = [vp, u32, ctypes.POINTER(u32 * 8)]
    L.sb_partition_layout.argtypes = [vp, ctypes.POINTER(u32)]
    L.sb_partition_rank_scene.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp]
    L.sb_partition_rank_ids.argtypes = [vp, u32, vp, vp, vp, vp]
    L.sb_partition_peer_counts.argtypes = [vp, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32 * 4)]
    L.sb_partition_peer_lists.argtypes = [vp, u32, u32, vp, vp, vp, vp]
    L.sb_partition_rank_guard.argtypes = [vp, u32, f32, vp, vp, vp, vp]
    L.sb_last_error.argtypes = [vp]
    L.sb_last_error.restype = ctypes.c_char_p
    L.sb_abi_version.restype = u32
    for name in declared_symbols():
        fn = getattr(L, name)
        if name not in ("sb_default_options", "sb_last_error", "sb_abi_version"):
            fn.restype = ctypes.c_int
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Engine(DeviceBinding):
    """Host-side handle of one engine; method names follow engineWorker.ts
    (writeBuffers / loadBuffers / frame) and the C ABI.

    Where a method takes device memory, device_binding.DeviceBinding checks it, orders the streams and binds a report's outputs,
    as it does for BatchEngine.  A bool is never a device pointer: ValueError, unless the method gives True / False a meaning of
    its own.  A tensor handed in with another shape than the documented one -- a flat one, say -- comes back as a view of the
    documented shape over the same storage; one that has the shape comes back as the same object."""

    def __init__(self, bounds_size=1000.0, particle_radius=10.0, subticks=64, layout=LAYOUT_V1,
                 max_particles=65536, max_beams=65536, collision_mode=COLLIDE_GRID,
                 path=PATH_AUTO, tile_particles=0, device=0, grid_skin=0.0, block_substeps=0):
        L = load_library()
        o = SbOptions()
        L.sb_default_options(ctypes.byref(o))
        o.bounds_size, o.particle_radius, o.subticks = bounds_size, particle_radius, subticks
        o.max_particles, o.max_beams, o.layout = max_particles, max_beams, layout
        o.collision_mode, o.path, o.tile_particles, o.device_ordinal = collision_mode, path, tile_particles, device
        o.grid_skin = grid_skin
        o.block_substeps = block_substeps
        self._h = ctypes.c_void_p()
        st = L.sb_create(ctypes.byref(o), ctypes.byref(self._h))
        if st != 0:
            self._h = None
            raise EngineError(st, L.sb_last_error(None).decode())
        self.layout, self.max_particles, self.max_beams = layout, max_particles, max_beams
        self.device = device
        self._ext_stream = None
        self.collision_mode = collision_mode
        self.subticks = (subticks + 1) // 2 * 2

    def _check(self, st):
        if st != 0:
            raise EngineError(st, load_library().sb_last_error(self._h).decode())

    def destroy(self):
        if self._h:
            load_library().sb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def write_buffers(self, buf: Buffers):
        self._check(load_library().sb_write_buffers(
            self._h, _ptr(buf.metadata), buf.metadata.nbytes, _ptr(buf.mapping), buf.mapping.nbytes,
            _ptr(buf.particles), buf.particles.nbytes, _ptr(buf.beams), buf.beams.nbytes))

    def load_buffers(self, buf: Buffers):
        self._check(load_library().sb_load_buffers(
            self._h, _ptr(buf.metadata), buf.metadata.nbytes, _ptr(buf.mapping), buf.mapping.nbytes,
            _ptr(buf.particles), buf.particles.nbytes, _ptr(buf.beams), buf.beams.nbytes))
        return buf

    def write_user_input(self, bytes32):
        b = (ctypes.c_ubyte * 32).from_buffer_copy(bytes32)
        self._check(load_library().sb_write_user_input(self._h, ctypes.cast(b, ctypes.c_void_p)))

    def set_physics_constants(self, consts8):
        a = np.asarray(consts8, dtype="<f4")
        assert a.shape == (8,)
        self._check(load_library().sb_set_physics_constants(self._h, _ptr(a)))

    def get_physics_constants(self):
        a = np.zeros(8, dtype="<f4")
        self._check(load_library().sb_get_physics_constants(self._h, _ptr(a)))
        return a

    def frame(self):
        self._check(load_library().sb_frame(self._h))

    def step(self, n):
        self._check(load_library().sb_step(self._h, n))

    def delete_pass(self):
        self._check(load_library().sb_delete_pass(self._h))

    def halo_delete_ghosts(self):
        self._check(load_library().sb_halo_delete_ghosts(self._h))

    def sync(self):
        self._check(load_library().sb_sync(self._h))

    def step_timed(self, n):
        ms = ctypes.c_float()
        self._check(load_library().sb_step_timed(self._h, n, ctypes.byref(ms)))
        return ms.value

    def mark(self, slot):
        """Record time mark `slot` at the current end of the engine's stream (does not wait)."""
        self._check(load_library().sb_mark(self._h, slot))

    def mark_elapsed(self, a, b):
        """Device milliseconds from mark a to mark b (waits for b)."""
        ms = ctypes.c_float()
        self._check(load_library().sb_mark_elapsed(self._h, a, b, ctypes.byref(ms)))
        return ms.value

    def counts(self):
        p, b = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(load_library().sb_get_counts(self._h, ctypes.byref(p), ctypes.byref(b)))
        return p.value, b.value

    def info(self, key):
        """sb_get_info: one counter or property of the engine by name (include/softbody.h lists them), e.g. "substeps_per_launch",
        "materials", "blocked_word_format" (0 wide, 1 narrow: how the blocked kernel holds the plan's entry words)."""
        v = ctypes.c_uint64()
        self._check(load_library().sb_get_info(self._h, key.encode(), ctypes.byref(v)))
        return v.value

    def kernel_name(self):
        """Name (up to the template arguments) of the kernel that does the substeps of this engine, as rocprofv3
        lists it."""
        if self.info("path") != PATH_TILED:
            return "k_beams_atomic+k_particles"
        if self.info("substeps_per_launch") > 1:
            return "k_substep_blocked"
        return "k_substep_tiled_grid" if self.collision_mode == COLLIDE_GRID else "k_substep_tiled"

    def sync_quiet(self):
        """sync() that swallows a reported device-side timeout (used when abandoning a failed exchange set-up)."""
        try:
            self.sync()
        except EngineError:
            pass

    def halo_configure(self, ghost_particles, send_particles, ghost_beams=(), send_beams=()):
        a = [np.ascontiguousarray(x, dtype="<u4") for x in (ghost_particles, send_particles, ghost_beams, send_beams)]
        self._check(load_library().sb_halo_configure(self._h, _ptr(a[0]), a[0].size, _ptr(a[1]), a[1].size,
                                                     _ptr(a[2]), a[2].size, _ptr(a[3]), a[3].size))

    def halo_set_layout(self, send_particle_off, send_beam_off, ghost_particle_off, ghost_beam_off):
        a = [np.ascontiguousarray(x, dtype="<u4") for x in (send_particle_off, send_beam_off, ghost_particle_off,
                                                             ghost_beam_off)]
        self._check(load_library().sb_halo_set_layout(self._h, *[_ptr(x) for x in a]))

    def peer_mailbox(self):
        """(local device pointer, 64-byte IPC handle, bytes) of this engine's mailbox (allocated on first call)."""
        ptr, nbytes = ctypes.c_void_p(), ctypes.c_uint64()
        handle = ctypes.create_string_buffer(64)
        self._check(load_library().sb_peer_mailbox(self._h, ctypes.byref(ptr), handle, ctypes.byref(nbytes)))
        return ptr.value, handle.raw, nbytes.value

    def peer_map(self, handle):
        ptr = ctypes.c_void_p()
        self._check(load_library().sb_peer_map(self._h, ctypes.c_char_p(bytes(handle)), ctypes.byref(ptr)))
        return ptr.value

    def peer_connect(self, mailboxes, peer_recv_floats, send_begin, send_len, dst_begin, their_slot, timeout_ms=0):
        n = len(mailboxes)
        boxes = (ctypes.c_void_p * max(n, 1))(*mailboxes)
        a = [np.ascontiguousarray(x, dtype="<u4") for x in (peer_recv_floats, send_begin, send_len, dst_begin, their_slot)]
        self._check(load_library().sb_peer_connect(self._h, n, boxes, *[_ptr(x) for x in a], int(timeout_ms)))

    def peer_exchange(self):
        self._check(load_library().sb_peer_exchange(self._h))

    def halo_pack(self, device_ptr):
        self._check(load_library().sb_halo_pack(self._h, ctypes.c_void_p(device_ptr)))

    def halo_unpack(self, device_ptr):
        self._check(load_library().sb_halo_unpack(self._h, ctypes.c_void_p(device_ptr)))

    def halo_guard(self, rank, world, depth, contact_reach, hop, lo, hi, own_particles, held, own_beams=(), motion=0.0):
        """sb_halo_guard: check the partition behind every ghost refresh from now on (include/softbody.h states the rule).
        own_particles / own_beams are LOCAL data indices, `held` the per-own-particle rank masks, lo / hi every rank's
        x-extent at partition time; motion = s per substep (0: the default H / (16 depth)).  Call after halo_configure."""
        op = np.ascontiguousarray(own_particles, dtype="<u4")
        hd = np.ascontiguousarray(held, dtype="<u8")
        ob = np.ascontiguousarray(own_beams, dtype="<u4")
        lo_, hi_ = np.ascontiguousarray(lo, dtype="<f4"), np.ascontiguousarray(hi, dtype="<f4")
        if hd.size != op.size or lo_.size != world or hi_.size != world:
            raise ValueError("halo_guard: held needs one mask per own particle, lo / hi one value per rank")
        d = SbHaloGuardDesc()
        d.struct_size = ctypes.sizeof(SbHaloGuardDesc)
        d.rank, d.world, d.depth = rank, world, depth
        d.contact_reach, d.hop, d.motion = contact_reach, hop, motion
        d.n_own_particles, d.own_particles, d.held = op.size, _ptr(op), _ptr(hd)
        d.n_own_beams, d.own_beams = ob.size, _ptr(ob)
        d.lo, d.hi = _ptr(lo_), _ptr(hi_)
        self._check(load_library().sb_halo_guard(self._h, ctypes.byref(d)))

    def halo_guard_off(self):
        self._check(load_library().sb_halo_guard(self._h, None))

    def halo_guard_status(self):
        """The guard's verdict so far (waits for the engine's stream): a GuardStatus."""
        r = SbHaloGuardReport()
        self._check(load_library().sb_halo_guard_status(self._h, ctypes.byref(r)))
        return GuardStatus(r)

    def stream(self):
        s = ctypes.c_void_p()
        self._check(load_library().sb_get_stream(self._h, ctypes.byref(s)))
        return s.value

    @staticmethod
    def _render_options(resolution, bounds_size, particle_radius):
        o = SbRenderOptions()
        o.struct_size = ctypes.sizeof(SbRenderOptions)
        o.resolution = int(resolution)
        o.bounds_size = 0.0 if bounds_size is None else float(bounds_size)
        o.particle_radius = 0.0 if particle_radius is None else float(particle_radius)
        return o

    def render(self, resolution=512, bounds_size=None, particle_radius=None):
        """The picture of host/render.js renderPPM (its body: RGB8, rows top to bottom) of the current state, drawn on the
        GPU: a (resolution, resolution, 3) uint8 array.  None = the engine's own bounds / radius.  Waits for the stream."""
        res = int(resolution)
        out = np.empty((res, res, 3), dtype=np.uint8)
        o = self._render_options(res, bounds_size, particle_radius)
        self._check(load_library().sb_render(self._h, ctypes.byref(o), _ptr(out), out.nbytes))
        return out

    def render_device(self, dst, resolution=512, bounds_size=None, particle_radius=None):
        """The same picture into device memory: `dst` is a device pointer (int) or a contiguous uint8 torch tensor of at least
        resolution^2 * 3 bytes on the engine's device.  Only enqueues on the engine's stream (sync() or the tensor's
        consumer ordered after stream() waits for it)."""
        res = int(resolution)
        if isinstance(dst, int):
            ptr = dst
        else:
            if not dst.is_contiguous() or dst.element_size() * dst.numel() < res * res * 3:
                raise ValueError("render_device: a contiguous tensor of at least %d bytes is needed" % (res * res * 3))
            ptr = dst.data_ptr()
        o = self._render_options(res, bounds_size, particle_radius)
        self._check(load_library().sb_render_device(self._h, ctypes.byref(o), ctypes.c_void_p(ptr)))

    # ---- the state in device memory (sb_read_state_device / sb_write_particles_device)

    def read_state_device(self, particles=None, beams=None, beam_alive=None):
        """The state sb_load_buffers would read back now, gathered on the GPU: particle records (6 f32: p.xy, v.xy, a.xy) at each
        particle's data index into `particles` (float32, max_particles * 24 bytes), {target_length, last_length, strain, stress}
        at each beam's data index into `beams` (float32, max_beams * 16 bytes), 1 / 0 (live / removed) into `beam_alive` (uint8,
        max_beams bytes).  Each is None, a device pointer (int) or a contiguous torch tensor on the engine's device; rows of no
        particle / beam are not written.  Only enqueues; with tensors, torch's current stream is ordered after the export."""
        args, tensors = [], False
        for what, x, dtype, n in (("particles", particles, "float32", self.max_particles * PARTICLE_STRIDE),
                                  ("beams", beams, "float32", self.max_beams * 16),
                                  ("beam_alive", beam_alive, "uint8", self.max_beams)):
            if x is None:
                args.append(None)
                continue
            ptr, t = self._device_buffer("read_state_device: " + what, x, dtype, n)
            args.append(ptr)
            tensors |= t
        vp = ctypes.c_void_p
        self._ordered(tensors, lambda: load_library().sb_read_state_device(self._h, vp(args[0]), vp(args[1]), vp(args[2])))

    def write_particles_device(self, src):
        """Overwrite p, v, a of every particle from particle records on the GPU (the layout of read_state_device's `particles`):
        a device pointer (int) or a contiguous float32 torch tensor of at least max_particles * 24 bytes on the engine's device.
        Only enqueues; with a tensor, the import waits for torch's current stream and torch's current stream for the import."""
        ptr, t = self._device_buffer("write_particles_device", src, "float32", self.max_particles * PARTICLE_STRIDE)
        self._ordered(t, lambda: load_library().sb_write_particles_device(self._h, ctypes.c_void_p(ptr)))

    def write_beams_device(self, src, target_length=True, last_length=False):
        """Overwrite target_length and / or last_length of every beam of the latest upload from beam rows on the GPU (the layout of
        read_state_device's `beams`: {target_length, last_length, strain, stress} at beam data indices; strain and stress are never
        imported): a device pointer (int) or a contiguous float32 torch tensor of at least max_beams * 16 bytes on the engine's
        device.  Every copy the engine keeps of a beam is written, bit for bit; a removed beam's row is written but inert.  Only
        enqueues; with a tensor, the import waits for torch's current stream and torch's current stream for the import."""
        fields = (BEAM_TARGET_LENGTH if target_length else 0) | (BEAM_LAST_LENGTH if last_length else 0)
        if not fields:
            raise ValueError("write_beams_device: neither target_length nor last_length is asked for")
        ptr, t = self._device_buffer("write_beams_device", src, "float32", self.max_beams * 16)
        self._ordered(t, lambda: load_library().sb_write_beams_device(self._h, ctypes.c_void_p(ptr), fields))

    def checkpoint(self):
        """Keep a copy of everything a run mutates in device memory of the engine's (one per engine: a later checkpoint replaces it;
        every write_buffers and halo_configure drops it).  Only enqueues (the first one after an upload allocates)."""
        self._check(load_library().sb_checkpoint_device(self._h))

    def restore(self):
        """Back to the checkpoint: every read-back, report and later step gives the bits the engine gave, or would have given, at
        and after checkpoint() -- also mid-frame and across delete passes.  Physics constants and user input stay as they are now.
        Only enqueues; EngineError (SB_ERR_STATE) without a checkpoint."""
        self._check(load_library().sb_restore_device(self._h))

    # ---- cutting beams on the device (sb_cut_device / sb_cut)

    @staticmethod
    def _cut_options(dry_run):
        o = SbCutOptions()
        o.struct_size = ctypes.sizeof(SbCutOptions)
        o.flags = CUT_DRY_RUN if dry_run else 0
        return o

    def cut(self, shapes, dry_run=False, hit=False, counts=True):
        """Cut the scene: every live beam that a shape hits (include/softbody.h states the predicate, on the positions at this
        point of the stream) gets its pending break flag raised, as if it had broken in the last substep -- it still acts until
        the next delete pass (frame()'s own, or delete_pass()), which removes it.  shapes: [n, 8] rows {kind, x0, y0, x1, y1, 0,
        0, 0}, n <= 64 (CUT_SEGMENT: a knife from (x0, y0) to (x1, y1); CUT_DISC: an eraser at (x0, y0) of radius x1; CUT_NONE:
        ignored) -- an int32 torch tensor on the engine's device (the coordinates as float bits; cut_shapes() packs such rows), a
        float32 tensor (the kind as a number: converted on the device), or a numpy array / list of (kind, x0, y0, x1, y1), which
        goes through sb_cut's checks on the host (that path waits for the stream).  dry_run: report, raise no flag.  Returns
        (hit, counts): hit uint8 [max_beams], 1 / 0 at the DATA index of every beam of the latest upload, indices of no beam not
        written (hit=True: a new zeroed tensor; a tensor / pointer: written into; False: None); counts int64 [4]
        (CUT_COUNT_FIELDS: tested, hit, flagged, already_flagged; False: None).  Tensors with device shapes, numpy arrays with
        host shapes.  Particles, beam floats, the spatial hash and the schedule are untouched."""
        o = self._cut_options(dry_run)
        vp = ctypes.c_void_p
        try:
            import torch
            on_device = isinstance(shapes, torch.Tensor)
        except ImportError:
            on_device = False
        if not on_device:
            rows = host_shapes(shapes)
            h = None
            if hit is not False:
                h = np.zeros(self.max_beams, dtype=np.uint8) if hit is True else hit
                if not (isinstance(h, np.ndarray) and h.dtype == np.uint8 and h.flags.c_contiguous and h.size >= self.max_beams):
                    raise ValueError("cut: with host shapes, hit is True or a contiguous uint8 numpy array of max_beams bytes")
            c = np.zeros(len(CUT_COUNT_FIELDS), dtype=np.int64) if counts is not False else None
            self._check(load_library().sb_cut(self._h, ctypes.byref(o), _ptr(rows) if len(rows) else None, len(rows), _ptr(h), _ptr(c)))
            return h, c
        dev = torch.device("cuda", self.device)
        words = device_shapes(shapes, dev)
        n = int(words.shape[0])
        if hit is None or counts is None:
            raise ValueError("cut: hit and counts are True, False, a device pointer (int) or a torch tensor, not None")
        zeroed = lambda: torch.zeros(self.max_beams, dtype=torch.uint8, device=dev)   # (indices of no beam are not written)
        outs, ptrs, _ = self._bind("cut", [
            ("hit", zeroed if hit is True else None if hit is False else hit, hit is not False, (self.max_beams,), "uint8"),
            ("counts", None if isinstance(counts, bool) else counts, counts is not False, (len(CUT_COUNT_FIELDS),), "int64")])
        self._ordered(True, lambda: load_library().sb_cut_device(self._h, ctypes.byref(o), vp(words.data_ptr() if n else None), n,
                                                                 vp(ptrs[0]), vp(ptrs[1])))
        return outs[0], outs[1]

    # ---- one summary row of the whole scene (sb_summary_device / sb_summary)

    @staticmethod
    def _summary_options(partials):
        o = SbSummaryOptions()
        o.struct_size = ctypes.sizeof(SbSummaryOptions)
        o.partials = int(partials)
        return o

    def summary(self, out=None, counts=None, partials=0):
        """One row of 24 statistics of the whole scene (SUMMARY_FIELDS names the words; the row of BatchEngine.summary(), bit for
        bit the same arithmetic), reduced on the GPU: a float32 tensor [24] on the engine's device.  `out`: a device pointer
        (int) or a contiguous float32 torch tensor of at least 24 elements to write into.  counts=True or an int64 tensor of at
        least 8 elements (or a device pointer): the exact integer counts too (SUMMARY_COUNT_FIELDS), returned as (row, counts).
        partials: where the reduction is cut (0: the engine's choice; the result does not depend on it).  Only reads the
        engine, only enqueues; torch's current stream is ordered after it."""
        want_counts = counts is not None and counts is not False
        (out, counts), (ptr, cptr), t = self._bind("summary", [
            ("out", out, True, (SUMMARY_WORDS,), "float32"),
            ("counts", None if isinstance(counts, bool) else counts, want_counts, (SUMMARY_COUNT_WORDS,), "int64")])
        o = self._summary_options(partials)
        vp = ctypes.c_void_p
        self._ordered(t, lambda: load_library().sb_summary_device(self._h, ctypes.byref(o), vp(ptr), vp(cptr)))
        return (out, counts) if want_counts else out

    def summary_host(self, partials=0):
        """The same row without torch: (float32 [24], uint64 [8]) numpy arrays.  Waits for the stream."""
        row = np.empty(SUMMARY_WORDS, dtype=np.float32)
        counts = np.empty(SUMMARY_COUNT_WORDS, dtype=np.uint64)
        o = self._summary_options(partials)
        self._check(load_library().sb_summary(self._h, ctypes.byref(o), _ptr(row), _ptr(counts)))
        return row, counts

    # ---- the connected bodies of the whole scene (sb_bodies_device / sb_bodies)

    def bodies(self, labels=None, sizes=False, counts=True):
        """The connected bodies of the scene: particles joined by LIVE beams (a pending break flag still connects; a beam removed
        by a delete pass, or by a plan-keeping upload that removed beams, does not), labelled on the GPU.  Returns
        (labels, counts), or (labels, counts, sizes) when sizes is asked for: torch tensors on the engine's device.  labels int32
        [max_particles]: at particle DATA index i (the rows of state_tensors()["particles"]) the smallest data index of i's body, -1
        where no particle lives -- what torch.index_add_ takes for a statistic per body.  counts int64 [4] (BODY_FIELDS names the
        words): bodies, particles of the largest, bodies of one particle, label of the largest (the smallest label on a tie;
        {0, 0, 0, -1} in a scene of no particles).  sizes int32 [max_particles, 2]: {particles, live beams} of the body at its
        label's row, {0, 0} in every other row.  Each argument: None or True -- a new tensor; False -- left out (None is
        returned in its place; not all three); a device pointer (int) or a contiguous torch tensor of that dtype and at least
        that many elements to write into.  Every word of an output is written.  Only reads the engine, only enqueues; torch's
        current stream is ordered after it."""
        outs, ptrs, tensors = self._bind("bodies", [
            (name, None if isinstance(x, bool) else x, x is not False, shape, dtype)   # (None / True: a new tensor)
            for name, x, shape, dtype in (("labels", labels, (self.max_particles,), "int32"), ("sizes", sizes, (self.max_particles, 2), "int32"),
                                          ("counts", counts, (BODY_WORDS,), "int64"))])
        vp = ctypes.c_void_p
        self._ordered(tensors, lambda: load_library().sb_bodies_device(self._h, None, vp(ptrs[0]), vp(ptrs[1]), vp(ptrs[2])))
        return (outs[0], outs[2], outs[1]) if sizes is not False else (outs[0], outs[2])

    def bodies_host(self):
        """The same without torch: (labels int32 [max_particles], sizes int32 [max_particles, 2], counts int64 [4]) numpy arrays.
        Waits for the stream."""
        labels = np.empty(self.max_particles, dtype=np.int32)
        sizes = np.empty((self.max_particles, 2), dtype=np.int32)
        counts = np.empty(BODY_WORDS, dtype=np.int64)
        self._check(load_library().sb_bodies(self._h, None, _ptr(labels), _ptr(sizes), _ptr(counts)))
        return labels, sizes, counts

    # ---- the beam graph of the whole scene (sb_graph_device / sb_graph)

    @staticmethod
    def _graph_options(max_half_edges, skip_pending):
        o = SbGraphOptions()
        o.struct_size = ctypes.sizeof(SbGraphOptions)
        o.flags = GRAPH_SKIP_PENDING if skip_pending else 0
        o.max_half_edges = int(max_half_edges)
        return o

    def graph(self, ends=True, adjacency=False, max_half_edges=None, skip_pending=False, counts=True):
        """The beam graph of the scene in the caller's index space, written on the GPU: (ends, row_ptr, nbr, counts), torch tensors
        on the engine's device, None where not asked for.  Nodes are the particles at particle DATA indices, edges the LISTED
        beams at beam DATA indices: the live beams by bodies()' rule (a pending break flag still connects), or with
        skip_pending=True those without a pending flag -- what the next delete pass will leave.  ends int32 [max_beams, 2]: {a, b} of
        the beam's record at its data index, (-1, -1) where no listed beam lives.  adjacency=True: row_ptr int64
        [max_particles + 1], the exclusive prefix sum of the degrees, always complete, and nbr int32 [max_half_edges, 2], the rows
        row_ptr[p] .. row_ptr[p + 1] - 1 being {other endpoint, beam data index} of the listed beams at p in ascending beam data
        index, (-1, -1) behind the last; max_half_edges=None: 2 * max_beams; 0: row_ptr alone.  counts int64 [4]
        (GRAPH_COUNT_FIELDS).  ends / counts: True, False, a device pointer (int) or a contiguous torch tensor to write into;
        adjacency: True, False or a pair (row_ptr, nbr) of those (then max_half_edges is nbr's rows).  Only reads the engine, only
        enqueues; torch's current stream is ordered after it."""
        import torch
        if isinstance(adjacency, (tuple, list)):
            row_ptr, nbr = adjacency
        else:
            row_ptr = nbr = bool(adjacency)
        H = 2 * self.max_beams if max_half_edges is None else int(max_half_edges)
        if isinstance(nbr, torch.Tensor) and max_half_edges is None:
            H = nbr.numel() // 2
        if H == 0:
            nbr = False
        if nbr is not False and nbr is not None and (row_ptr is False or row_ptr is None):
            raise ValueError("graph: nbr without row_ptr")
        outs, ptrs, tensors = self._bind("graph", [
            (name, None if isinstance(x, bool) else x, x is not False and x is not None, shape, dtype)   # (True: a new tensor)
            for name, x, shape, dtype in (("ends", ends, (self.max_beams, 2), "int32"), ("row_ptr", row_ptr, (self.max_particles + 1,), "int64"),
                                          ("nbr", nbr, (H, 2), "int32"), ("counts", counts, (GRAPH_COUNT_WORDS,), "int64"))])
        o = self._graph_options(H if ptrs[2] else 0, skip_pending)
        vp = ctypes.c_void_p
        self._ordered(tensors, lambda: load_library().sb_graph_device(self._h, ctypes.byref(o), vp(ptrs[0]), vp(ptrs[1]), vp(ptrs[2]), vp(ptrs[3])))
        return tuple(outs)

    def graph_host(self, max_half_edges=None, skip_pending=False):
        """The same without torch: (ends, row_ptr, nbr, counts) numpy arrays (nbr None with max_half_edges=0).  Waits for the stream."""
        H = 2 * self.max_beams if max_half_edges is None else int(max_half_edges)
        ends = np.empty((self.max_beams, 2), dtype=np.int32)
        row_ptr = np.empty(self.max_particles + 1, dtype=np.int64)
        nbr = np.empty((H, 2), dtype=np.int32) if H else None
        counts = np.empty(GRAPH_COUNT_WORDS, dtype=np.int64)
        o = self._graph_options(H, skip_pending)
        self._check(load_library().sb_graph(self._h, ctypes.byref(o), _ptr(ends), _ptr(row_ptr), _ptr(nbr), _ptr(counts)))
        return ends, row_ptr, nbr, counts

    # ---- range sensors over the whole scene (sb_raycast_device / sb_raycast)

    @staticmethod
    def _raycast_options(cells_per_side):
        o = SbRaycastOptions()
        o.struct_size = ctypes.sizeof(SbRaycastOptions)
        o.cells_per_side = int(cells_per_side)
        return o

    def raycast(self, rays, labels=None, t=None, hit=None, counts=None, cells_per_side=0):
        """"How far is the nearest thing in this direction, and what is it?" asked of the whole scene, on the GPU: BatchEngine.raycast()'s
        definition, bit for bit, on what load_buffers() would return now.  `rays` is [n, 8], n <= 2^24, in sb_batch_ray's layout
        {mask, ox, oy, dx, dy, tmax, skip_label, 0}: an int32 or float32 (bits) torch tensor on the engine's device (ray_rows() packs
        one), or a tuple (device pointer, n).  Returns a RayCast named tuple of tensors on the engine's device: t [n] float32; hit
        [n, 3] int32 (batch.RAY_HIT_FIELDS: kind, particle / beam DATA index or WALL_* word, label); counts [8] int64
        (RAYCAST_COUNT_FIELDS: valid rows, hits on particles, beams and walls, then the cost words -- rows answered by the sweep over
        every primitive, particles outside the grid, long beams: every ray is tested against each of the last two).  labels: None,
        True (self.bodies() runs first, on the same stream, and its labels are used), or an int32 tensor / device pointer of
        [max_particles] labels of the caller's own, only compared.  t / hit / counts: None or True -- a new tensor; False -- left out
        (None in its place; not all three); a device pointer (int) or a contiguous torch tensor to write into.  cells_per_side: 0 =
        the engine's rule (info("raycast_cells_per_side")); the outputs do not depend on it.  Only reads the engine, only
        enqueues; torch's current stream is ordered after it."""
        import torch
        if isinstance(rays, tuple):
            rptr, n = int(rays[0]), int(rays[1])
            is_tensor = False
        else:
            if not isinstance(rays, torch.Tensor) or rays.dtype not in (torch.int32, torch.float32) or rays.dim() != 2 or rays.shape[1] != 8:
                raise ValueError("raycast: rays must be an int32 / float32 torch tensor [n, 8] or (device pointer, n)")
            n = int(rays.shape[0])
            rptr, is_tensor = self._device_buffer("raycast: rays", rays, None, n * 32)
        if not 0 <= n <= RAYCAST_MAX_RAYS:
            raise ValueError("raycast: %d rays, not in 0 .. 2^24" % n)
        wanted = [x is not False for x in (t, hit, counts)]
        if not any(wanted):
            raise ValueError("raycast: t, hit and counts are all False: nothing to write")
        given = [None if isinstance(x, bool) else x for x in (t, hit, counts)]   # (None / True: a new tensor)
        outs, ptrs, tensors = self._bind("raycast", [
            ("t", given[0], wanted[0], (n,), "float32"),
            ("hit", given[1], wanted[1], (n, 3), "int32"),
            ("counts", given[2], wanted[2], (RAYCAST_COUNT_WORDS,), "int64"),
            ("labels", (lambda: self.bodies(counts=False)[0]) if labels is True else None if labels is False else labels,
             labels is not None and labels is not False, (self.max_particles,), "int32")])
        if n == 0:   # (the library enqueues nothing for no rays: the counts of no rays are zeros)
            if isinstance(outs[2], torch.Tensor):
                outs[2].zero_()
            return RayCast(*outs[:3])
        o = self._raycast_options(cells_per_side)
        vp = ctypes.c_void_p
        self._ordered(tensors or is_tensor, lambda: load_library().sb_raycast_device(self._h, ctypes.byref(o), vp(rptr), n, vp(ptrs[3]), vp(ptrs[0]),
                                                                                     vp(ptrs[1]), vp(ptrs[2])))
        return RayCast(*outs[:3])

    def raycast_host(self, rays, labels=None, cells_per_side=0):
        """The same without torch: rays a uint32 / int32 / float32 (bits) numpy array [n, 8], labels None or int32 [max_particles];
        returns RayCast(t float32 [n], hit int32 [n, 3], counts int64 [8]) numpy arrays.  Waits for the stream."""
        rows = np.ascontiguousarray(rays)
        if rows.dtype not in (np.dtype(np.uint32), np.dtype(np.int32), np.dtype(np.float32)) or rows.ndim != 2 or rows.shape[1] != 8:
            raise ValueError("raycast_host: rays must be a uint32 / int32 / float32 array [n, 8]")
        n = rows.shape[0]
        t, hit, counts = np.zeros(n, dtype=np.float32), np.zeros((n, 3), dtype=np.int32), np.zeros(RAYCAST_COUNT_WORDS, dtype=np.int64)
        lab = None
        if labels is not None:
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            if lab.size < self.max_particles:
                raise ValueError("raycast_host: labels needs max_particles entries")
        o = self._raycast_options(cells_per_side)
        self._check(load_library().sb_raycast(self._h, ctypes.byref(o), _ptr(rows) if n else None, n, None if lab is None else _ptr(lab), _ptr(t),
                                              _ptr(hit), _ptr(counts)))
        return RayCast(t, hit, counts)

    # ---- proximity queries over the whole scene (sb_nearest_device / sb_nearest)

    @staticmethod
    def _nearest_options(cells_per_side, max_rings):
        o = SbNearestOptions()
        o.struct_size = ctypes.sizeof(SbNearestOptions)
        o.cells_per_side, o.max_rings = int(cells_per_side), int(max_rings)
        return o

    def nearest(self, points, labels=None, d=None, hit=None, point=None, within=None, counts=None, cells_per_side=0, max_rings=0):
        """"What is nearest to this point, how far is it, and how much is within reach?" asked of the whole scene, on the GPU:
        BatchEngine.nearest()'s definition, bit for bit, on what load_buffers() would return now.  `points` is [n, 8], n <= 2^24, in
        sb_batch_near_point's layout {mask, px, py, rmax, skip_label, 0, 0, 0}: an int32 or float32 (bits) torch tensor on the
        engine's device, or a tuple (device pointer, n).  batch.point_rows() already packs such rows on the device: give it [1, n, 2]
        points and take [0].  Returns a Nearest named tuple of tensors on the engine's device: d [n] float32; hit [n, 3] int32
        (batch.NEAR_HIT_FIELDS: kind, particle / beam DATA index or WALL_* word, label); point [n, 2] float32, the closest point on
        the winner; within [n, 2] int32, particles and beams within rmax; counts [8] int64 (NEAREST_COUNT_FIELDS: valid rows, winners
        that are particles, beams and walls, then the cost words -- rows answered by the sweep over every primitive, particles
        outside the grid, long beams).  labels: None, True (self.bodies() runs first, on the same stream), or an int32 tensor / device
        pointer of [max_particles] labels of the caller's own, only compared.  d / hit / point / within / counts: None or True -- a
        new tensor; False -- left out (None in its place; not all five); a device pointer (int) or a contiguous torch tensor to
        write into.  Leaving `within` out lets a row stop at its winner: with rmax = inf it is the difference between a few cells
        and a pass over the scene.  cells_per_side: 0 = the engine's rule (info("nearest_cells_per_side")); max_rings: 0 = the
        default (info("nearest_max_rings")); the outputs depend on neither.  Only reads the engine, only enqueues; torch's current
        stream is ordered after it.

        Hover, then grab, without leaving the device:
            rows = batch.point_rows(cursor[None], rmax=3 * radius, mask=batch.NEAR_PARTICLES)[0]    # cursor: [n, 2] on the device
            near = eng.nearest(rows, within=False, counts=False)
            st = eng.state_tensors()["particles"]                                                  # [max_particles, ...] at data indices
            grabbed = near.hit[:, 0] == 1
            st[near.hit[grabbed, 1].long(), :2] = cursor[grabbed]
            eng.write_particles_device(st)"""
        import torch
        if isinstance(points, tuple):
            rptr, n = int(points[0]), int(points[1])
            is_tensor = False
        else:
            if not isinstance(points, torch.Tensor) or points.dtype not in (torch.int32, torch.float32) or points.dim() != 2 or points.shape[1] != 8:
                raise ValueError("nearest: points must be an int32 / float32 torch tensor [n, 8] or (device pointer, n)")
            n = int(points.shape[0])
            rptr, is_tensor = self._device_buffer("nearest: points", points, None, n * 32)
        if not 0 <= n <= NEAREST_MAX_POINTS:
            raise ValueError("nearest: %d points, not in 0 .. 2^24" % n)
        asked = (d, hit, point, within, counts)
        wanted = [x is not False for x in asked]
        if not any(wanted):
            raise ValueError("nearest: d, hit, point, within and counts are all False: nothing to write")
        given = [None if isinstance(x, bool) else x for x in asked]   # (None / True: a new tensor)
        outs, ptrs, tensors = self._bind("nearest", [
            ("d", given[0], wanted[0], (n,), "float32"),
            ("hit", given[1], wanted[1], (n, 3), "int32"),
            ("point", given[2], wanted[2], (n, 2), "float32"),
            ("within", given[3], wanted[3], (n, 2), "int32"),
            ("counts", given[4], wanted[4], (NEAREST_COUNT_WORDS,), "int64"),
            ("labels", (lambda: self.bodies(counts=False)[0]) if labels is True else None if labels is False else labels,
             labels is not None and labels is not False, (self.max_particles,), "int32")])
        if n == 0:   # (the library enqueues nothing for no points: the counts of no points are zeros)
            if isinstance(outs[4], torch.Tensor):
                outs[4].zero_()
            return Nearest(*outs[:5])
        o = self._nearest_options(cells_per_side, max_rings)
        vp = ctypes.c_void_p
        self._ordered(tensors or is_tensor, lambda: load_library().sb_nearest_device(self._h, ctypes.byref(o), vp(rptr), n, vp(ptrs[5]), vp(ptrs[0]),
                                                                                     vp(ptrs[1]), vp(ptrs[2]), vp(ptrs[3]), vp(ptrs[4])))
        return Nearest(*outs[:5])

    def nearest_host(self, points, labels=None, cells_per_side=0, max_rings=0):
        """The same without torch: points a uint32 / int32 / float32 (bits) numpy array [n, 8], labels None or int32 [max_particles];
        returns Nearest(d float32 [n], hit int32 [n, 3], point float32 [n, 2], within int32 [n, 2], counts int64 [8]) numpy arrays.
        Waits for the stream."""
        rows = np.ascontiguousarray(points)
        if rows.dtype not in (np.dtype(np.uint32), np.dtype(np.int32), np.dtype(np.float32)) or rows.ndim != 2 or rows.shape[1] != 8:
            raise ValueError("nearest_host: points must be a uint32 / int32 / float32 array [n, 8]")
        n = rows.shape[0]
        out = Nearest(np.zeros(n, dtype=np.float32), np.zeros((n, 3), dtype=np.int32), np.zeros((n, 2), dtype=np.float32),
                      np.zeros((n, 2), dtype=np.int32), np.zeros(NEAREST_COUNT_WORDS, dtype=np.int64))
        lab = None
        if labels is not None:
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            if lab.size < self.max_particles:
                raise ValueError("nearest_host: labels needs max_particles entries")
        o = self._nearest_options(cells_per_side, max_rings)
        self._check(load_library().sb_nearest(self._h, ctypes.byref(o), _ptr(rows) if n else None, n, None if lab is None else _ptr(lab),
                                              *(_ptr(x) for x in out)))
        return out

    # ---- particle and wall contacts of the whole scene (sb_contacts_device / sb_contacts)

    @staticmethod
    def _contacts_options(max_pairs, other_body):
        o = SbContactsOptions()
        o.struct_size = ctypes.sizeof(SbContactsOptions)
        o.flags = CONTACTS_OTHER_BODY if other_body else 0
        o.max_pairs = int(max_pairs)
        return o

    def contacts(self, labels=None, pairs=0, other_body=False, touch=True, counts=True, out=None):
        """Who touches whom, and who touches a wall, in the whole scene, found on the GPU.  Two particles touch iff the next
        substep's collision loop would act on them (dist == 0 or dist < 2 * particle_radius in the library's float arithmetic); the
        answer is the same in every collision_mode and on every path.  Returns (touch, counts), or (touch, counts, pairs) when a
        pair list is asked for: torch tensors on the engine's device.  touch int32 [max_particles, 4] at particle DATA indices
        (CONTACT_TOUCH_FIELDS names the columns): particles touching i, those of them whose label differs from i's (-1 without
        labels), the wall bits (WALL_LEFT x <= r, WALL_RIGHT x >= bounds - r, WALL_LOW y <= r, WALL_HIGH y >= bounds - r), the
        smallest data index touching i (-1: none); a row where no particle lives is (0, 0 or -1, 0, -1).  counts int64 [4]
        (CONTACT_COUNT_FIELDS): touching pairs (the true number, however short the list), pairs of different labels (-1 without
        labels), particles on a wall, particles touching another.  pairs int32 [n, 2]: the pairs (i, j), i < j, in ascending
        order of (i, j), the first n of them, (-1, -1) behind the last; with other_body=True only pairs of different labels.
        labels: None, True (self.bodies() is called first, on the same stream, and its labels are used), or an int32 tensor /
        device pointer of [max_particles] labels of the caller's own, which are only compared with each other.  pairs: 0 / None
        = no list; n = a list of n pairs (a new tensor, or `out`: a device pointer or a contiguous int32 tensor of at least
        2 n elements to write into); or such a tensor itself, n = its pairs.  touch / counts: None or True -- a new tensor;
        False -- left out (None is returned in its place); a device pointer (int) or a contiguous torch tensor of that dtype
        and at least that many elements to write into.  Every word of an output is written.  Only reads the engine, only
        enqueues; torch's current stream is ordered after it."""
        import torch
        maxp = self.max_particles
        if isinstance(pairs, torch.Tensor):
            if out is not None:
                raise ValueError("contacts: pairs is a tensor to write into, and so is out")
            out, pairs = pairs, pairs.numel() // 2
        elif pairs is None:
            pairs = 0
        if isinstance(pairs, bool) or not isinstance(pairs, (int, np.integer)) or pairs < 0:
            raise ValueError("contacts: pairs is a number of pairs or an int32 torch tensor, not %r" % (pairs,))
        max_pairs = int(pairs)
        if out is not None and max_pairs == 0:
            raise ValueError("contacts: out needs a pair list (pairs > 0)")
        outs, ptrs, tensors = self._bind("contacts", [
            ("touch", None if isinstance(touch, bool) else touch, touch is not False, (maxp, CONTACT_WORDS), "int32"),
            ("counts", None if isinstance(counts, bool) else counts, counts is not False, (CONTACT_COUNT_WORDS,), "int64"),
            ("pairs", out, max_pairs > 0, (max_pairs, 2), "int32"),
            ("labels", (lambda: self.bodies(counts=False)[0]) if labels is True else None if labels is False else labels,
             labels is not None and labels is not False, (maxp,), "int32")])
        o = self._contacts_options(max_pairs, other_body)
        vp = ctypes.c_void_p
        self._ordered(tensors, lambda: load_library().sb_contacts_device(self._h, ctypes.byref(o), vp(ptrs[3]), vp(ptrs[0]), vp(ptrs[2]),
                                                                         vp(ptrs[1])))
        return (outs[0], outs[1], outs[2]) if max_pairs > 0 else (outs[0], outs[1])

    def contacts_host(self, labels=None, pairs=0, other_body=False):
        """The same without torch: (touch int32 [max_particles, 4], counts int64 [4], pairs int32 [pairs, 2]) numpy arrays; labels:
        None or an int32 array of [max_particles] labels.  Waits for the stream."""
        touch = np.empty((self.max_particles, CONTACT_WORDS), dtype=np.int32)
        counts = np.empty(CONTACT_COUNT_WORDS, dtype=np.int64)
        plist = np.empty((int(pairs), 2), dtype=np.int32)
        lab = None
        if labels is not None:
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            if lab.size < self.max_particles:
                raise ValueError("contacts_host: labels needs max_particles entries")
        o = self._contacts_options(pairs, other_body)
        self._check(load_library().sb_contacts(self._h, ctypes.byref(o), None if lab is None else _ptr(lab), _ptr(touch),
                                               _ptr(plist) if int(pairs) else None, _ptr(counts)))
        return touch, counts, plist

    # ---- beam and contact forces of the whole scene (sb_forces_device / sb_forces)

    @staticmethod
    def _forces_options(other_body):
        o = SbForcesOptions()
        o.struct_size = ctypes.sizeof(SbForcesOptions)
        o.flags = FORCES_OTHER_BODY if other_body else 0
        return o

    def forces(self, labels=None, other_body=False, rows=True, beam_i32=None, tension=None, counts=None):
        """How hard every beam pulls and every contact pushes in the whole scene, found on the GPU: the forces the NEXT substep
        would compute from the CURRENT state, in the step's own arithmetic, bit for bit (include/softbody.h states the definition:
        BatchEngine.forces()' for one scene).  Nothing is applied: no yield, no last_length update, no break flag, no particle moved.
        Returns batch.Forces, a named tuple of tensors on the engine's device (None where not asked for):
        rows [max_particles, 8] float32 at particle DATA indices (FORCE_FIELDS names the columns): beam_x, beam_y, the sum of the beam
        forces on the particle (the fixed-point sum times 2^-16, what the integration adds to the acceleration); push_x, push_y, what
        the contacts add to the acceleration; impulse_x, impulse_y, what they add to the velocity; depth, the largest overlap 2r -
        dist among the partners; partners, their number.  Eight zeros where no particle lives.
        beam_i32 [max_particles, 2] int32: the fixed-point beam force sums themselves (wrapping, saturating).
        tension [max_beams] float32 at beam DATA indices (the rows of state_tensors()'s beams): the beam's force_mag, positive when the
        beam is compressed and pushes its endpoints apart, negative when it is stretched and pulls; 0 where no live beam is.  A beam
        with a pending break flag still pulls; one a delete pass or an upload removed does not.
        counts [4] int64 (FORCE_COUNT_FIELDS): particles, beams evaluated, particles with a partner, beams whose tension is not finite.
        labels: None, True (self.bodies() is called first, on the same stream, and its labels are used), or an int32 tensor / device
        pointer of [max_particles] labels of the caller's own; with other_body=True only partners whose label differs from the
        particle's are taken: what another body does to this one.  rows / beam_i32 / tension / counts: True (a new tensor), None /
        False (not wanted), a device pointer (int) or a contiguous torch tensor to write into; every word of what is asked for is
        written.  Only reads the engine, only enqueues; torch's current stream is ordered after it."""
        from .batch import Forces
        maxp, maxb = self.max_particles, self.max_beams
        wanted = [x is not False and x is not None for x in (rows, beam_i32, tension, counts)]
        given = [None if isinstance(x, bool) else x for x in (rows, beam_i32, tension, counts)]   # (True: a new tensor)
        outs, ptrs, tensors = self._bind("forces", [
            ("rows", given[0], wanted[0], (maxp, FORCE_WORDS), "float32"),
            ("beam_i32", given[1], wanted[1], (maxp, 2), "int32"),
            ("tension", given[2], wanted[2], (maxb,), "float32"),
            ("counts", given[3], wanted[3], (FORCE_COUNT_WORDS,), "int64"),
            ("labels", (lambda: self.bodies(counts=False)[0]) if labels is True else None if labels is False else labels,
             labels is not None and labels is not False, (maxp,), "int32")])
        o = self._forces_options(other_body)
        vp = ctypes.c_void_p
        self._ordered(tensors, lambda: load_library().sb_forces_device(self._h, ctypes.byref(o), vp(ptrs[4]), *[vp(p) for p in ptrs[:4]]))
        return Forces(*outs[:4])

    def forces_host(self, labels=None, other_body=False):
        """The same without torch: batch.Forces of numpy arrays (rows float32 [max_particles, 8], beam_i32 int32 [max_particles, 2],
        tension float32 [max_beams], counts int64 [4]); labels: None or an int32 array of [max_particles] labels.  Waits for the
        stream."""
        from .batch import Forces
        rows = np.empty((self.max_particles, FORCE_WORDS), dtype=np.float32)
        beam_i32 = np.empty((self.max_particles, 2), dtype=np.int32)
        tension = np.empty(self.max_beams, dtype=np.float32)
        counts = np.empty(FORCE_COUNT_WORDS, dtype=np.int64)
        lab = None
        if labels is not None:
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            if lab.size < self.max_particles:
                raise ValueError("forces_host: labels needs max_particles entries")
        o = self._forces_options(other_body)
        self._check(load_library().sb_forces(self._h, ctypes.byref(o), None if lab is None else _ptr(lab), _ptr(rows), _ptr(beam_i32),
                                             _ptr(tension), _ptr(counts)))
        return Forces(rows, beam_i32, tension, counts)

    # ---- statistics per body of the whole scene (sb_body_summary_device / sb_body_summary)

    def _body_summary_options(self, what, rows):
        if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or not 1 <= rows <= self.max_particles:
            raise ValueError("%s: rows is %r, not a number in 1 .. max_particles (%d)" % (what, rows, self.max_particles))
        o = SbBodySummaryOptions()
        o.struct_size = ctypes.sizeof(SbBodySummaryOptions)
        o.max_rows = int(rows)
        return o

    def body_summary(self, labels=None, rows=8, out=None, counts=False, rank=False):
        """One row of 24 statistics per GROUP of particles of the whole scene (BODY_SUMMARY_FIELDS names the columns; the row of
        BatchEngine.body_summary(), the same definition): a float32 tensor [rows, 24] on the engine's device -- alone, or followed
        by counts and / or rank, in that order, where they are asked for.  labels: None or True (self.bodies()' labelling runs
        first, on the same stream, and the groups are the bodies) or an int32 tensor / device pointer of [max_particles] labels of
        the caller's own at particle DATA indices: a value 0 .. max_particles-1 names the particle's group, any other value puts it
        into none; a live beam belongs to the group that holds both its endpoints.  Row k is the group of rank k -- particles
        descending, then label ascending -- and rows behind the last group are empty (label -1, counts 0, NaN elsewhere).  Counts,
        label, pending breaks, means, extremes, kinetic energy and angular momentum of the group's finite particles, strain and
        stress extremes of its finite beams; the sums are those of summary()'s pinned tree over the group alone, so a row is the
        same bits on every run, and a scene that is one body gives summary()'s words.  counts int64 [rows, 8]
        (BODY_SUMMARY_COUNT_FIELDS): the integers of a row exactly, whatever the size of the scene.  rank int32 [max_particles]:
        the rank of the group of the particle at that data index (>= rows: its row was cut), -1 where no particle lives or the
        particle is in no group.  rows: 1 .. max_particles.  out: None or True -- a new tensor; False -- left out (None in its
        place; not all three); counts / rank: False -- left out; None or True -- a new tensor; each also a device pointer (int)
        or a contiguous torch tensor of that dtype and at least that many elements to write into.  Every word of an output is
        written.  Only reads the engine, only enqueues; torch's current stream is ordered after it."""
        o = self._body_summary_options("body_summary", rows)
        rows = int(rows)
        want_counts, want_rank = counts is not False, rank is not False
        own = labels is not None and labels is not True   # (the engine's bodies are labelled inside the call: no buffer of the caller's)
        outs, ptrs, tensors = self._bind("body_summary", [
            (name, None if isinstance(x, bool) else x, x is not False, shape, dtype)   # (None / True: a new tensor)
            for name, x, shape, dtype in (("out", out, (rows, BODY_SUMMARY_WORDS), "float32"),
                                          ("counts", counts, (rows, BODY_SUMMARY_COUNT_WORDS), "int64"),
                                          ("rank", rank, (self.max_particles,), "int32"))]
            + [("labels", labels if own else None, own, (self.max_particles,), "int32")])
        vp = ctypes.c_void_p
        self._ordered(tensors, lambda: load_library().sb_body_summary_device(self._h, ctypes.byref(o), vp(ptrs[3]), vp(ptrs[0]), vp(ptrs[1]),
                                                                             vp(ptrs[2])))
        res = [outs[0]] + ([outs[1]] if want_counts else []) + ([outs[2]] if want_rank else [])
        return res[0] if len(res) == 1 else tuple(res)

    def body_summary_host(self, labels=None, rows=8):
        """The same without torch: (rows float32 [rows, 24], counts int64 [rows, 8], rank int32 [max_particles]) numpy arrays;
        labels: None (the engine's bodies) or an int32 array of [max_particles] labels.  Waits for the stream."""
        o = self._body_summary_options("body_summary_host", rows)
        out = np.empty((int(rows), BODY_SUMMARY_WORDS), dtype=np.float32)
        counts = np.empty((int(rows), BODY_SUMMARY_COUNT_WORDS), dtype=np.int64)
        rank = np.empty(self.max_particles, dtype=np.int32)
        lab = None
        if labels is not None:
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            if lab.size < self.max_particles:
                raise ValueError("body_summary_host: labels needs max_particles entries")
        self._check(load_library().sb_body_summary(self._h, ctypes.byref(o), None if lab is None else _ptr(lab), _ptr(out), _ptr(counts),
                                                   _ptr(rank)))
        return out, counts, rank

    def state_tensors(self):
        """New torch tensors of the current state: {"particles": (max_particles, 6) float32, "beams": (max_beams, 4) float32,
        "beam_alive": (max_beams,) uint8}; rows of no particle / beam are NaN (0 in beam_alive)."""
        import torch
        dev = torch.device("cuda", self.device)
        out = {"particles": torch.full((self.max_particles, 6), float("nan"), dtype=torch.float32, device=dev),
               "beams": torch.full((self.max_beams, 4), float("nan"), dtype=torch.float32, device=dev),
               "beam_alive": torch.zeros(self.max_beams, dtype=torch.uint8, device=dev)}
        self.read_state_device(out["particles"], out["beams"], out["beam_alive"])
        return out
