"""sb_batch_fork_device / _checkpoint_device / _write_beams_device without a GPU: declared, exported, bound with prototypes, argument
errors before a device is looked for, and every scene and program of tests/test_gpu_fork.py keeps the ORACLE finite.  The beam
import's expected values rest on the oracle's load_buffers -> write_buffers round trip being bit-neutral where the GPU test uses
it (at frame boundaries): asserted here."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
import batch_fork_cases as fc  # noqa: E402
import batch_grid_cases as gc  # noqa: E402

SYMBOLS = ["sb_batch_fork_device", "sb_batch_checkpoint_device", "sb_batch_write_beams_device"]


def test_header_declares_and_library_exports_the_three_calls(sb):
    names = sb.engine.declared_symbols()
    L = sb.batch.load_library()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    for s in SYMBOLS:
        assert s in names, s
        assert hasattr(L, s), s
        assert getattr(L, s).restype is ctypes.c_int, s
    assert L.sb_batch_fork_device.argtypes == [vp, vp, u32]
    assert L.sb_batch_checkpoint_device.argtypes == [vp, vp]
    assert L.sb_batch_write_beams_device.argtypes == [vp, vp, u32]
    assert L.sb_abi_version() == 1   # additions only
    for m in ("fork", "checkpoint", "write_beams_device"):
        assert callable(getattr(sb.BatchEngine, m)), m
    assert sb.batch.FORK_KEEP == 0xFFFFFFFF == fc.KEEP
    assert (sb.batch.FORK_CONSTANTS, sb.batch.FORK_AS_RESET, sb.batch.BEAM_TARGET_LENGTH, sb.batch.BEAM_LAST_LENGTH) == (1, 2, 1, 2)
    header = open(sb.engine.HEADER_PATH).read()
    for needle in ("#define SB_BATCH_FORK_KEEP 0xFFFFFFFFu", "#define SB_BATCH_FORK_CONSTANTS 1u", "#define SB_BATCH_FORK_AS_RESET 2u",
                   "#define SB_BATCH_BEAM_TARGET_LENGTH 1u", "#define SB_BATCH_BEAM_LAST_LENGTH 2u", "fork_staging_bytes", "fork_bad_sources"):
        assert needle in header, needle


def test_argument_errors_are_invalid_before_anything_touches_a_device(sb):
    """NULL handle, NULL pointer, bad flags / fields: SB_ERR_INVALID on a machine without a GPU too."""
    L = sb.batch.load_library()
    word = (ctypes.c_uint32 * 4)()
    p = ctypes.cast(word, ctypes.c_void_p)
    assert L.sb_batch_fork_device(None, None, 0) == 1 and L.sb_batch_fork_device(None, p, 0) == 1 and L.sb_batch_fork_device(None, p, 4) == 1
    assert L.sb_batch_checkpoint_device(None, None) == 1 and L.sb_batch_checkpoint_device(None, p) == 1
    assert L.sb_batch_write_beams_device(None, None, 1) == 1 and L.sb_batch_write_beams_device(None, p, 0) == 1
    assert L.sb_batch_write_beams_device(None, p, 4) == 1 and L.sb_batch_write_beams_device(None, p, 3) == 1


def test_python_refuses_what_is_not_a_buffer(sb):
    be = sb.BatchEngine.__new__(sb.BatchEngine)
    be._h, be.device, be.n_scenes, be.max_particles, be.max_beams, be._ext_stream = None, 0, 2, 16, 16, None
    import torch
    for call in (lambda: be.fork("no"), lambda: be.fork([0, 1]), lambda: be.fork(torch.zeros(2, dtype=torch.int32)),
                 lambda: be.checkpoint("no"), lambda: be.checkpoint(torch.zeros(2, dtype=torch.uint8)),
                 lambda: be.write_beams_device("no"), lambda: be.write_beams_device(torch.zeros((2, 16, 4)))):
        with pytest.raises(ValueError):
            call()


def assert_finite(refs, what):
    for i, r in enumerate(refs):
        if r is not None:
            assert fc.is_finite(r), "%s: scene %d is not finite" % (what, i)


@pytest.mark.parametrize("which", ["hetero", "break"])
def test_broadcast_programs_stay_finite_and_have_flags_pending(sb, oracle, which):
    """2 frames + step(5), then (after the fork) delete_pass + 2 frames, on the source scene."""
    case = bc.case_hetero(sb) if which == "hetero" else bc.case_break(sb)
    k = 1 if which == "hetero" else 4
    refs = [None] * len(case["bufs"])
    refs[k] = bc.make_oracle(oracle, case, case["bufs"][k])
    fc.advance(refs, [op for op in case["program"] if op[0] == "consts"] + [("frame", 2), ("step", 5)])
    assert_finite(refs, which + " at the fork")
    if which == "break":
        assert refs[k].delete.any(), "flags must be pending at the fork"
        assert int(refs[k].metadata[6]) < case["bufs"][k].beam_count, "the forked state must have removed beams"
    fc.advance(refs, [("delete",), ("frame", 2)])
    assert_finite(refs, which + " at the end")


def test_snapshot_keep_and_constants_programs_stay_finite(sb, oracle):
    for n, sources in ((64, [s for _, s in fc.snapshot_sources(64)]), (8, [fc.KEEP_SOURCES])):
        case = fc.case_distinct(sb, n)
        refs = bc.run_oracles(oracle, case)
        states = {r.particles_a.tobytes() + r.particles_b.tobytes() for r in refs}
        assert len(states) == n, "the scenes must be distinct"
        for src in sources:
            refs = fc.fork_oracles(refs, src)
            fc.advance(refs, [("frame", 1)])
            assert_finite(refs, "distinct x %d" % n)
    case = fc.case_consts(sb)
    for constants in (False, True):
        refs = fc.fork_oracles(bc.run_oracles(oracle, case), fc.CONSTS_SOURCES, constants)
        fc.advance(refs, [("frame", 1)])
        assert_finite(refs, "constants=%s" % constants)
    a, b = (fc.fork_oracles(bc.run_oracles(oracle, case), fc.CONSTS_SOURCES, c) for c in (False, True))
    fc.advance(a + b, [("frame", 1)])
    assert not np.array_equal(a[0].particles_a, b[0].particles_a), "the constants must matter"


def test_checkpoint_program_stays_finite(sb, oracle):
    """test_checkpoint_and_reset's oracle side, step for step."""
    case = bc.case_break(sb)
    bufs = case["bufs"]
    n = len(bufs)
    more, rest = [("frame", 1), ("step", 5)], [("step", 59), ("delete",), ("frame", 1)]
    refs = [bc.make_oracle(oracle, case, b) for b in bufs]
    fc.advance(refs, [("frame", 2)])
    assert any(int(r.metadata[6]) < b.beam_count for r, b in list(zip(refs, bufs))[0::2]), "a masked scene must have lost beams"
    saved = [fc.clone(r) for r in refs]
    fc.advance(refs, more)
    for i in (0, 2, 4):
        refs[i] = fc.clone(saved[i])
    refs[1] = bc.make_oracle(oracle, case, bufs[1])
    fc.advance(refs, more)
    assert any(r.delete.any() for r in refs), "flags must be pending at checkpoint(None)"
    saved = [fc.clone(r) for r in refs]
    fc.advance(refs, rest)
    assert_finite(refs, "past checkpoint(None)")
    refs = [fc.clone(r) for r in saved]
    fc.advance(refs, rest)
    refs = fc.fork_oracles(refs, [4] * n)
    fc.advance(refs, [("frame", 1)])
    refs = [refs[2] if i == 2 else fc.clone(saved[4]) for i in range(n)]
    fc.advance(refs, rest)
    assert_finite(refs, "after the plain fork")
    assert not np.array_equal(refs[2].particles_a, refs[0].particles_a) or not np.array_equal(refs[2].particles_b, refs[0].particles_b)
    mid = fc.clone(refs[2])
    refs = [fc.clone(mid) for _ in range(n)]
    fc.advance(refs, [("frame", 1), ("step", 3)])
    assert_finite(refs, "after fork(as_reset)")
    refs = [fc.clone(saved[4]) if i == 2 else fc.clone(mid) for i in range(n)]
    fc.advance(refs, [("frame", 1)])
    assert_finite(refs, "a frame after the last reset")


def test_beam_import_program_stays_finite_and_the_round_trip_is_bit_neutral(sb, oracle):
    case = fc.beam_case(sb)
    n, tpl = len(case["bufs"]), case["bufs"][0]
    refs = bc.run_oracles(oracle, case)
    fc.advance(refs, [("frame", 1)])
    # load_buffers -> write_buffers with nothing changed, at a frame boundary: later frames keep their bits
    plain = [fc.clone(r) for r in refs]
    for r in refs:
        assert not r.delete.any()
        r.write_buffers(r.load_buffers(tpl.copy()))
    fc.advance(refs + plain, [("frame", 2)])
    for i, (r, p) in enumerate(zip(refs, plain)):
        bc.assert_same(r.load_buffers(tpl.copy()), p.load_buffers(tpl.copy()), "round trip, scene %d" % i)
    refs = bc.run_oracles(oracle, case)
    fc.advance(refs, [("frame", 1)])
    factors = fc.beam_factors(n, tpl.max_beams)
    assert (factors != 1.0).any() and len({f.tobytes() for f in factors}) == n
    for target, last in fc.BEAM_ROUNDS:
        rows = fc.edit_beams(np.stack([fc.export_of(r, tpl) for r in refs]), factors, target, last)
        before = [fc.clone(r) for r in refs]
        for i, r in enumerate(refs):
            fc.import_into_oracle(r, tpl, rows[i], target, last)
        fc.advance(refs + before, [("frame", 1)])
        assert_finite(refs, "beam import %s" % ((target, last),))
        assert all(not np.array_equal(r.particles_a, b.particles_a) or not np.array_equal(r.particles_b, b.particles_b)
                   for r, b in zip(refs, before)), "the edit must matter"


def test_identity_import_case_has_flags_pending_and_rows_without_effect(sb, oracle):
    """case_break after 2 frames + step(5): flags are pending, beams have been removed, and the capacity has data indices
    without a beam; the continuation (step(59), delete_pass, a frame) stays finite."""
    case = bc.case_break(sb)
    refs = [bc.make_oracle(oracle, case, b) for b in case["bufs"]]
    fc.advance(refs, [("frame", 2), ("step", 5)])
    assert any(r.delete.any() for r in refs)
    assert any(int(r.metadata[6]) < b.beam_count for r, b in zip(refs, case["bufs"]))
    assert all(b.beam_count < b.max_beams for b in case["bufs"])
    fc.advance(refs, [("step", 59), ("delete",), ("frame", 1)])
    assert_finite(refs, "identity import")


def test_pile_program_stays_finite(sb, oracle):
    """step(7), the fork, step(57) + delete_pass + step(5): case_pile's own frame + step(5) for every scene."""
    case = gc.case_pile(sb)
    assert case["program"] == [("frame", 1), ("step", 5)] and case["cap"] == (256, 0)
    refs = [gc.make_oracle(oracle, case, case["bufs"][0])]
    fc.advance(refs, [("step", 7), ("step", 57), ("delete",), ("step", 5)])
    assert_finite(refs, "pile")
