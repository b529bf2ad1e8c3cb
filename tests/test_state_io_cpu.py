"""sb_read_state_device / sb_write_particles_device without a GPU: softbody.h declares both, engine.py binds them with prototypes,
and the Engine methods exist (test_abi_cpu.py::test_library_exports_every_declared_symbol then covers the library's exports)."""
import ctypes

import pytest


def test_header_declares_state_io(sb):
    names = sb.engine.declared_symbols()
    assert "sb_read_state_device" in names and "sb_write_particles_device" in names


def test_engine_binds_state_io(sb):
    L = sb.engine.load_library()
    vp = ctypes.c_void_p
    assert L.sb_read_state_device.argtypes == [vp, vp, vp, vp]
    assert L.sb_write_particles_device.argtypes == [vp, vp]
    assert L.sb_read_state_device.restype is ctypes.c_int and L.sb_write_particles_device.restype is ctypes.c_int
    # a NULL engine is refused before anything touches a device
    assert L.sb_read_state_device(None, None, None, None) == 1
    assert L.sb_write_particles_device(None, None) == 1
    for m in ("read_state_device", "write_particles_device", "state_tensors"):
        assert callable(getattr(sb.Engine, m))


@pytest.mark.parametrize("name", ["read_state_device", "write_particles_device"])
def test_methods_refuse_what_is_not_a_buffer(sb, name):
    """The argument check comes before any call into the library (no engine needed: the check does not touch the handle)."""
    eng = sb.Engine.__new__(sb.Engine)
    eng._h, eng.device, eng.max_particles, eng.max_beams, eng._ext_stream = None, 0, 16, 16, None
    with pytest.raises(ValueError):
        getattr(eng, name)("not a buffer")
