"""sb_write_beams_device / sb_checkpoint_device / sb_restore_device without a GPU: softbody.h declares them, engine.py binds them with
prototypes, the SB_BEAM_* constants agree between the header and Python, and the argument checks that come before any device call."""
import ctypes
import re

import pytest

SYMBOLS = ["sb_write_beams_device", "sb_checkpoint_device", "sb_restore_device"]


def test_header_declares_the_three_calls(sb):
    names = sb.engine.declared_symbols()
    for s in SYMBOLS:
        assert s in names, s


def test_constants_agree(sb):
    src = open(sb.engine.HEADER_PATH).read()
    got = {n: int(v) for n, v in re.findall(r"#define SB_BEAM_(TARGET_LENGTH|LAST_LENGTH)\s+(\d+)u", src)}
    assert got == {"TARGET_LENGTH": sb.engine.BEAM_TARGET_LENGTH, "LAST_LENGTH": sb.engine.BEAM_LAST_LENGTH} == {"TARGET_LENGTH": 1, "LAST_LENGTH": 2}
    assert (sb.engine.BEAM_TARGET_LENGTH, sb.engine.BEAM_LAST_LENGTH) == (sb.batch.BEAM_TARGET_LENGTH, sb.batch.BEAM_LAST_LENGTH)


def test_engine_binds_them(sb):
    L = sb.engine.load_library()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert L.sb_write_beams_device.argtypes == [vp, vp, u32]
    assert L.sb_checkpoint_device.argtypes == [vp] and L.sb_restore_device.argtypes == [vp]
    for s in SYMBOLS:
        assert getattr(L, s).restype is ctypes.c_int
    for m in ("write_beams_device", "checkpoint", "restore"):
        assert callable(getattr(sb.Engine, m))


def test_null_engine_is_refused_without_a_device(sb):
    L = sb.engine.load_library()
    p = ctypes.c_void_p(4096)
    assert L.sb_checkpoint_device(None) == 1 and L.sb_restore_device(None) == 1
    for src, fields in ((None, 1), (p, 0), (p, 4), (p, 3)):
        assert L.sb_write_beams_device(None, src, fields) == 1


def test_write_beams_device_rejects_both_fields_false(sb):
    """The check comes before any call into the library (no engine needed), and before the buffer is looked at."""
    eng = sb.Engine.__new__(sb.Engine)
    eng._h, eng.device, eng.max_particles, eng.max_beams, eng._ext_stream = None, 0, 16, 16, None
    with pytest.raises(ValueError, match="neither"):
        eng.write_beams_device(4096, target_length=False, last_length=False)
    with pytest.raises(ValueError):
        eng.write_beams_device("not a buffer")
