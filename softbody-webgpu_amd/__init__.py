"""softbody-webgpu_amd: MI355X-native drop-in for the physics step of spsquared/softbody-webgpu.

The directory name carries a hyphen (it is the reference's name), so load it with
`__graft_entry__.load_package()` or importlib; inside, modules use relative imports.

  layout.py   host-visible byte layouts (mirror of src/engineMapping.ts)
  scenes.py   synthetic scene generators (generalised main.ts:addRectangle)
  engine.py   ctypes binding of the C ABI in include/softbody.h (libsoftbody_hip.so)
  batch.py    BatchEngine: the sb_batch_* group (N small scenes, one workgroup each, one launch per frame)
  device_binding.py   what Engine and BatchEngine share for device memory: buffer check, stream ordering, output binder
  csrc/       HIP kernels + the C ABI + the N-API addon
  host/       JavaScript/TypeScript host mirror of engine.ts / engineMapping.ts / engineWorker.ts
"""
from . import layout, scenes  # noqa: F401
from .layout import LAYOUT_V1, LAYOUT_V2, Buffers  # noqa: F401


def __getattr__(name):
    if name in ("engine", "Engine", "EngineError", "halo", "batch", "BatchEngine"):
        import importlib
        mod = importlib.import_module({"halo": ".halo", "batch": ".batch", "BatchEngine": ".batch"}.get(name, ".engine"), __name__)
        return mod if name in ("engine", "halo", "batch") else getattr(mod, name)
    if name in ("BODY_SUMMARY_FIELDS", "BODY_SUMMARY_COUNT_FIELDS",  # the words of Engine.body_summary()'s rows and counts
                "CUT_NONE", "CUT_SEGMENT", "CUT_DISC", "CUT_COUNT_FIELDS", "cut_shapes"):  # Engine.cut() / BatchEngine.cut()
        from . import engine
        return getattr(engine, name)
    if name in ("GRAPH_COUNT_FIELDS", "GRAPH_MATERIAL_FIELDS",  # the words of BatchEngine.graph()'s counts and material rows
                "RAY_HIT_FIELDS", "RAY_COUNT_FIELDS", "ray_rows",  # BatchEngine.raycast()
                "NEAR_HIT_FIELDS", "NEAR_WITHIN_FIELDS", "NEAR_COUNT_FIELDS", "point_rows",  # BatchEngine.nearest()
                "SPAWN_EMPTY", "SPAWN_INVALID", "SPAWN_BLOCKED", "SPAWN_FULL", "SPAWN_COUNT_FIELDS",  # BatchEngine.add_particles()
                "POSE_FIELDS", "POSE_MOMENT_FIELDS", "pose_fit"):  # BatchEngine.pose()
        from . import batch
        return getattr(batch, name)
    raise AttributeError(name)
