"""The sb_batch_* group without a GPU: the header declares it, the library exports it, batch.py binds it with prototypes,
option errors are reported before a device is looked for, and every scene and seed tests/test_gpu_batch.py uses keeps the
ORACLE finite to the last checkpoint (so that no GPU case needs a skip or an early break)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402

SYMBOLS = ["sb_batch_default_options", "sb_batch_create", "sb_batch_destroy", "sb_batch_write_scene", "sb_batch_write_user_input",
           "sb_batch_write_user_input_device", "sb_batch_set_physics_constants", "sb_batch_frame", "sb_batch_step",
           "sb_batch_delete_pass", "sb_batch_reset_device", "sb_batch_read_state_device", "sb_batch_write_particles_device",
           "sb_batch_load_scene", "sb_batch_sync", "sb_batch_get_stream", "sb_batch_get_info", "sb_batch_last_error"]


def has_gpu():
    import torch
    return torch.cuda.is_available()


def default_options(sb):
    L = sb.batch.load_library()
    o = sb.batch.SbBatchOptions()
    L.sb_batch_default_options(ctypes.byref(o))
    return L, o


def test_header_declares_and_library_exports_the_batch_group(sb):
    names = sb.engine.declared_symbols()
    L = sb.batch.load_library()
    for s in SYMBOLS:
        assert s in names, s
        assert hasattr(L, s), s
    assert L.sb_abi_version() == 1   # additions only


def test_batch_py_binds_with_prototypes(sb):
    L = sb.batch.load_library()
    vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    assert L.sb_batch_write_scene.argtypes == [vp, u32, u32, vp, sz, vp, sz, vp, sz, vp, sz]
    assert L.sb_batch_load_scene.argtypes == [vp, u32, vp, sz, vp, sz, vp, sz, vp, sz]
    assert L.sb_batch_frame.argtypes == [vp, u32] and L.sb_batch_step.argtypes == [vp, u32]
    assert L.sb_batch_read_state_device.argtypes == [vp, vp, vp, vp]
    assert L.sb_batch_last_error.restype is ctypes.c_char_p and L.sb_batch_default_options.restype is None
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None, s
        if s not in ("sb_batch_default_options", "sb_batch_last_error"):
            assert getattr(L, s).restype is ctypes.c_int, s
    for m in ("write_scene", "write_user_input", "set_physics_constants", "frame", "step", "delete_pass", "reset", "state_tensors",
              "read_state_device", "write_particles_device", "load_scene", "sync", "info", "destroy", "stream"):
        assert callable(getattr(sb.BatchEngine, m)), m
    assert sb.BatchEngine is sb.batch.BatchEngine


def test_null_handle_is_invalid_before_anything_touches_a_device(sb):
    L = sb.batch.load_library()
    assert L.sb_batch_destroy(None) == 1
    assert L.sb_batch_write_scene(None, 0, 1, None, 0, None, 0, None, 0, None, 0) == 1
    assert L.sb_batch_write_user_input(None, None) == 1 and L.sb_batch_write_user_input_device(None, None) == 1
    assert L.sb_batch_set_physics_constants(None, 0, 1, None) == 1
    assert L.sb_batch_frame(None, 1) == 1 and L.sb_batch_step(None, 1) == 1 and L.sb_batch_delete_pass(None) == 1
    assert L.sb_batch_reset_device(None, None) == 1
    assert L.sb_batch_read_state_device(None, None, None, None) == 1 and L.sb_batch_write_particles_device(None, None) == 1
    assert L.sb_batch_load_scene(None, 0, None, 0, None, 0, None, 0, None, 0) == 1
    assert L.sb_batch_sync(None) == 1 and L.sb_batch_get_stream(None, None) == 1 and L.sb_batch_get_info(None, b"n_scenes", None) == 1


def test_default_options(sb):
    L, o = default_options(sb)
    assert o.struct_size == ctypes.sizeof(sb.batch.SbBatchOptions) == 64
    assert (o.n_scenes, o.bounds_size, o.particle_radius, o.subticks, o.layout) == (1, 1000.0, 10.0, 64, 1)
    assert (o.max_particles, o.max_beams) == (sb.batch.BATCH_MAX_PARTICLES, sb.batch.BATCH_MAX_BEAMS)
    assert o.max_particles >= 1024 and o.max_beams >= 4096          # a full-density lattice in the reference's box
    assert o.collision_mode != 0


@pytest.mark.parametrize("field,value,needle", [("max_particles", 1025, b"1024"), ("max_beams", 4097, b"4096"),
                                                ("n_scenes", 0, b"n_scenes is 0"), ("struct_size", 8, b"8"),
                                                ("max_beams", 70000, b"65536"), ("max_particles", 70000, b"65536")])
def test_bad_options_are_invalid_with_the_number_in_the_message(sb, field, value, needle):
    """Options are checked BEFORE a device is looked for: SB_ERR_INVALID on a machine without a GPU too."""
    L, o = default_options(sb)
    setattr(o, field, value)
    h = ctypes.c_void_p()
    assert L.sb_batch_create(ctypes.byref(o), ctypes.byref(h)) == 1
    assert needle in L.sb_batch_last_error(None), L.sb_batch_last_error(None)
    assert not h.value


def test_capacity_error_reaches_python_with_the_limit(sb):
    with pytest.raises(sb.EngineError) as ei:
        sb.BatchEngine(n_scenes=4, max_particles=2048, max_beams=64)
    assert ei.value.status == 1 and "1024" in str(ei.value)


def test_no_device_no_fallback(sb):
    """Valid options on a machine without a GPU: SB_ERR_NO_DEVICE (with a GPU the batch is simply created)."""
    gpu = has_gpu()
    try:
        be = sb.BatchEngine(n_scenes=2, max_particles=128, max_beams=320)
    except sb.EngineError as e:
        assert not gpu and e.status == 3 and "no CPU fallback" in str(e)
    else:
        assert gpu
        assert be.info("scene_max_particles") >= 1024 and be.info("scene_max_beams") >= 4096
        be.destroy()


def test_python_refuses_what_is_not_a_buffer(sb):
    be = sb.BatchEngine.__new__(sb.BatchEngine)
    be._h, be.device, be.n_scenes, be.max_particles, be.max_beams, be._ext_stream = None, 0, 2, 16, 16, None
    for call in (lambda: be.write_particles_device("no"), lambda: be.read_state_device("no"), lambda: be.reset("no"),
                 lambda: be.write_user_input(b"short")):
        with pytest.raises(ValueError):
            call()


def test_every_gpu_case_keeps_the_oracle_finite(sb, oracle):
    """A condition, not a measurement: every scene and seed of tests/test_gpu_batch.py, through its whole program, stays finite
    in the oracle at every checkpoint; zero cases are skipped or cut short."""
    for case in bc.all_cases(sb):
        def finite(refs, k, case=case):
            for i, ref in enumerate(refs):
                if ref is not None:
                    cur = ref.particles_b if ref.final_in_b else ref.particles_a
                    assert np.isfinite(cur).all(), "%s: scene %d is not finite after op %d" % (case["name"], i, k)
        refs = bc.run_oracles(oracle, case, finite)
        assert any(r is not None for r in refs)


def test_break_case_removes_beams_in_some_scenes_only(sb, oracle):
    """The yield / break case must exercise the delete pass in at least one scene and leave at least one scene whole."""
    case = bc.case_break(sb)
    refs = bc.run_oracles(oracle, case)
    removed = [b.beam_count - int(r.metadata[6]) for b, r in zip(case["bufs"], refs)]
    assert max(removed) > 0 and min(removed) == 0, removed


def test_mapping_case_is_what_it_says(sb):
    perm, co = bc.case_mapping(sb)["bufs"]
    P = perm.particle_count
    assert not np.array_equal(perm.mapping[:P], np.arange(P))
    pos = co.particles[co.mapping[:co.particle_count].astype(np.int64), :2]
    assert (pos[0] == pos[1]).all() and (pos[2] == pos[3]).all() and (pos[3] == pos[4]).all()
    assert list(np.argsort(co.mapping[:6])) != list(range(6))      # the data-index order is not the slot order
