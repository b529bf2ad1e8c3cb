"""sb_batch_forces_device without a GPU: declared, exported, bound; its argument errors before a device is looked for; the numpy
restatement (tests/batch_forces_ref.py) on a scene worked out by hand; three wrong variants of it told apart by the cases of
tests/batch_forces_cases.py; the restatement anchored on the oracle (one substep: v = (push + beam) * 2^-6, stress = tension / 20);
csrc/sb_batch_forces_math.h on the host under sanitizers (tests/batch_forces_check.cpp) against the restatement, bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
import batch_forces_cases as fc  # noqa: E402
import batch_grid_cases as gc  # noqa: E402
import batch_forces_ref as fr  # noqa: E402
from test_hostcheck_cpu import CSRC  # noqa: E402

F = np.float32


def u4(a):
    return fr.words(a)


# ---------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_the_call(sb):
    names = sb.engine.declared_symbols()
    L = sb.batch.load_library()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert "sb_batch_forces_device" in names and hasattr(L, "sb_batch_forces_device")
    assert L.sb_batch_forces_device.restype is ctypes.c_int and L.sb_batch_forces_device.argtypes == [vp, u32, vp, vp, vp, vp, vp]
    assert L.sb_abi_version() == 1   # additions only
    header = open(sb.engine.HEADER_PATH).read()
    for needle in ("#define SB_BATCH_FORCE_WORDS 8u", "#define SB_BATCH_FORCE_COUNT_WORDS 4u", "#define SB_BATCH_FORCES_OTHER_BODY 1u",
                   "forces_kernel_vgprs", "forces_kernel_scratch_bytes", "_forces_device only ENQUEUE"):
        assert needle in header, needle


def test_python_has_the_call_and_the_constants(sb):
    b = sb.batch
    assert callable(sb.BatchEngine.forces)
    assert b.FORCE_WORDS == fr.WORDS == 8 == len(b.FORCE_FIELDS) and b.FORCE_FIELDS == fr.FIELDS
    assert b.FORCE_COUNT_FIELDS == ("particles", "beams", "touching_particles", "nonfinite_beams") and len(b.FORCE_COUNT_FIELDS) == fr.COUNT_WORDS
    assert b.FORCES_OTHER_BODY == 1 and b.Forces._fields == ("rows", "beam_i32", "tension", "counts")


def test_argument_errors_come_before_any_device(sb):
    L = sb.batch.load_library()
    word = (ctypes.c_int32 * 32)()
    p = ctypes.cast(word, ctypes.c_void_p)
    assert L.sb_batch_forces_device(None, 0, None, None, None, None, None) == 1
    assert L.sb_batch_forces_device(None, 0, p, p, p, p, p) == 1
    assert b"sb_batch_forces_device: null batch" in L.sb_batch_last_error(None)
    # (no batch exists without a device, so the flag, label and alignment checks are exercised on a live handle by
    # tests/test_gpu_batch_forces.py::test_argument_errors; here only the handle check can be reached)


# ---------------------------------------------------------------- the restatement by hand
def test_restatement_on_the_scene_worked_out_by_hand(sb):
    """Slots 0, 1 hold data indices 5, 2 at (100, 200), (140, 200); the beam a = 5, b = 2 has target 30, last 38, spring 2, damp
    0.5: len = 40, force_mag = (30 - 40) * 2 + (38 - 40) * 0.5 = -21 (stretched: negative, it pulls the endpoints together),
    n = (40 * (1 / 40), 0) = (1, 0) in float32, f = (-21, 0); b gets i32(-21 * 65536) = -1376256, a the negative."""
    buf = fc.hand_scene(sb)
    rows, beam_i32, tension, counts = fr.forces_ref(buf)
    assert rows.dtype == tension.dtype == F and beam_i32.dtype == counts.dtype == np.int32
    assert F(40.0) * (F(1.0) / F(40.0)) == F(1.0)
    assert beam_i32[5].tolist() == [1376256, 0] and beam_i32[2].tolist() == [-1376256, 0]
    assert rows[5].tolist() == [21.0, 0.0, 0, 0, 0, 0, 0, 0] and rows[2].tolist() == [-21.0, 0.0, 0, 0, 0, 0, 0, 0]
    assert tension.tolist() == [-21.0] + [0.0] * 7 and counts.tolist() == [2, 1, 0, 0]
    live = np.zeros(8, bool)
    live[[5, 2]] = True
    assert not u4(rows[~live]).any() and not beam_i32[~live].any()
    # 25 apart instead: still no contact; 19 apart: one partner each, depth 1, push 0.5 * 4096 = 2048 away from the other
    buf.particles[2, 0] = 119.0
    rows = fr.forces_ref(buf)[0]
    assert rows[5, 2:].tolist() == [-2048.0, 0.0, 0.0, 0.0, 1.0, 1.0] and rows[2, 2:].tolist() == [2048.0, 0.0, 0.0, 0.0, 1.0, 1.0]
    buf.particle_count = 0
    assert all(not u4(x).any() for x in fr.forces_ref(buf))


def test_conversion_is_v_cvt_i32_f32(oracle):
    xs = np.array([0.0, -0.0, 0.9, -0.9, 1.5, -1.5, 2147483520.0, 2147483648.0, -2147483648.0, -2147483904.0, 1e30, -1e30, np.inf, -np.inf,
                   np.nan], F)
    want = [oracle.lib().sbo_f32_to_i32(float(x)) for x in xs]
    assert fr.f32_to_i32(xs).tolist() == want
    assert want[7] == 2 ** 31 - 1 and want[8] == -2 ** 31 and want[-1] == 0


# ---------------------------------------------------------------- the restatement bites
def test_descending_order_differs_on_the_five_partners(sb):
    buf = fc.contact_zoo(sb)
    d0 = int(buf.mapping[0])
    good, bad = fr.forces_ref(buf)[0], fr.forces_ref(buf, descending=True)[0]
    assert good[d0, 7] == 5.0 and good[d0, 6] > 19.9
    assert (u4(good[d0, 2:6]) != u4(bad[d0, 2:6])).any()
    assert np.array_equal(u4(good[:, 6:]), u4(bad[:, 6:])) and np.array_equal(u4(good[:, :2]), u4(bad[:, :2]))


def test_no_saturation_differs_on_the_saturating_star(sb):
    buf = fc.star(sb, 1e9)
    good, bad = fr.forces_ref(buf), fr.forces_ref(buf, saturate=False)
    assert not np.array_equal(good[1], bad[1])
    centre = int(buf.mapping[0])
    assert good[1][centre, 0] == -64                                  # 64 times INT_MAX, wrapped: 64 * (2^31 - 1) = -64 (mod 2^32)
    assert {int(v) for v in good[1][buf.mapping[1:64].astype(int), 0]} <= {-2 ** 31, 0}          # (joined twice: 2 * INT_MIN wraps to 0)
    # the gentler star wraps without saturating: the true sum is beyond 2^31
    gentle = fc.star(sb, 20.0)
    _, words = fr.beam_eval(*_beam_inputs(gentle))
    assert (np.abs(words.astype(np.int64)) < 2 ** 31 - 1).all() and abs(int(words[:, 0].astype(np.int64).sum())) > 2 ** 31
    assert np.array_equal(fr.forces_ref(gentle)[1], fr.forces_ref(gentle, saturate=False)[1])


def _beam_inputs(buf):
    bd = buf.mapping[buf.max_particles:buf.max_particles + buf.beam_count].astype(int)
    rec = buf.beams[bd]
    pa, pb = buf.particles[rec["a"].astype(int)], buf.particles[rec["b"].astype(int)]
    return pa[:, 0], pa[:, 1], pb[:, 0], pb[:, 1], rec["target_length"], rec["last_length"], rec["spring"], rec["damp"]


def test_skipping_pending_beams_differs(sb):
    buf = fc.beam_kinds(sb)
    good, bad = fr.forces_ref(buf), fr.forces_ref(buf, skip_slots=(0,))
    assert not np.array_equal(u4(good[0]), u4(bad[0])) and good[3].tolist() == [6, 3, 0, 0] and bad[3].tolist() == [6, 2, 0, 0]
    assert good[2][0] != 0 and bad[2][0] == 0


def test_the_cases_hold_what_they_promise(sb):
    kinds = fr.forces_ref(fc.beam_kinds(sb))
    assert kinds[2][0] < 0 < kinds[2][1] and kinds[2][2] == 0.0            # stretched, compressed, at rest
    odd = fr.forces_ref(fc.odd_beams(sb))
    assert odd[3].tolist() == [6, 3, 2, 1] and np.isnan(odd[2][1]) and not odd[1][[2, 3]].any()
    assert odd[1][4].tolist() == [2 ** 31 - 1, 0] and odd[1][5].tolist() == [-2 ** 31, 0]
    assert odd[1][0].tolist()[0] == 0 and odd[1][0].tolist()[1] != 0      # the beam of length zero pushes along -y
    assert odd[0][0, 6] == 20.0 and odd[0][0, 7] == 1.0 and not u4(odd[0][0, 2:6]).any()       # and its endpoints sit on one spot
    zoo = fc.contact_zoo(sb)
    rows = fr.forces_ref(zoo)[0]
    d = zoo.mapping[:16].astype(int)
    assert rows[d[6], 7] == 0 and rows[d[7], 7] == 0 and rows[d[8], 7] == 1 and rows[d[9], 7] == 1      # exactly 2r apart; an ulp closer
    assert rows[d[10], 7] == 0 and rows[d[12], 7] == 1 and rows[d[14]].tolist()[2:] == [0, 0, 0, 0, 20.0, 1.0]
    assert u4(rows[d[0], 4:6]).all()                                       # moving partners: impulse
    assert fr.forces_ref(fc.contact_zoo(sb, -1))[3][0] == 15 and fr.forces_ref(zoo)[3][0] == 16 == fc.GRID_MIN
    assert fr.inv_dt2_of(64) == (F(4096.0), F(2.0 ** -12)) and fr.inv_dt2_of(60)[0] == 0.0
    r64, r60 = fr.forces_ref(zoo, subticks=64)[0], fr.forces_ref(zoo, subticks=60)[0]
    assert not np.array_equal(u4(r64[:, 2:4]), u4(r60[:, 2:4])) and np.array_equal(u4(r64[:, 4:]), u4(r60[:, 4:]))
    crowd = fc.crowded_cell(sb)
    g, cell = gc.cell_geometry(1000.0, 10.0, fc.CONTACT_CAP[0])
    per_cell = lambda b: np.unique((b.particles[b.mapping[:b.particle_count].astype(int), :2] / cell).astype(int), axis=0, return_counts=True)[1].max()
    assert g == 49 and per_cell(crowd) == 5 > gc.CELL_K and per_cell(zoo) <= gc.CELL_K and rows[d[0], 7] == 5 > 4      # (two sweeps)
    assert per_cell(fc.case_full_width(sb)["bufs"][0]) <= gc.CELL_K
    two, D, body = __import__("batch_contacts_cases").two_bodies(sb)
    lab = np.full(two.max_particles, -1, np.int32)
    lab[D] = body
    every, cross = fr.forces_ref(two, labels=lab)[0], fr.forces_ref(two, labels=lab, other_body=True)[0]
    assert every[:, 7].sum() == 44 and cross[:, 7].sum() == 6 and fr.forces_ref(two, labels=lab, other_body=True)[3][2] == 6


# ---------------------------------------------------------------- the oracle anchor
@pytest.mark.parametrize("name", ["beams only", "contacts only", "both"])
def test_one_oracle_substep_is_the_restatement(sb, oracle, name):
    buf = fc.anchor_scenes(sb)[name]
    rows, beam_i32, tension, counts = fr.forces_ref(buf)
    assert (counts[1] > 0) == (name != "contacts only") and (counts[2] > 0) == (name != "beams only")
    ref = oracle.OracleEngine(1000.0, 10.0, 64, buf.layout, oracle.COLLIDE_ALLPAIRS)
    ref.write_buffers(buf)
    ref.step(1)
    after = ref.load_buffers(buf.copy())
    assert np.isfinite(after.particles).all()
    idx = buf.mapping[:buf.particle_count].astype(int)
    lo, hi = 10.0, 990.0
    assert ((after.particles[idx, :2] > lo) & (after.particles[idx, :2] < hi)).all()         # nobody met a wall
    want_v = (rows[idx, 2:4] + rows[idx, 0:2]) * F(2.0 ** -6)
    assert want_v.dtype == F and np.abs(want_v).max() > 0
    assert np.array_equal(u4(after.particles[idx, 2:4]), u4(want_v)), name
    bd = buf.mapping[buf.max_particles:buf.max_particles + buf.beam_count].astype(int)
    assert np.array_equal(u4(after.beams["stress"][bd]), u4(tension[bd] * fr.STRESS_SCALE)), name


# ---------------------------------------------------------------- the header's math under sanitizers
def _records(sb):
    bufs = [fc.contact_zoo(sb), fc.crowded_cell(sb), fc.contact_zoo(sb, 2, consts=dict(friction=0.7, elasticity=0.9)),
            fc.anchor_scenes(sb)["contacts only"]]
    beams = [fc.beam_kinds(sb), fc.star(sb, 20.0), fc.star(sb, 1e9), fc.odd_beams(sb), bc.saturation_scene(sb), sb.scenes.default_buffers(2, 128, 320)]
    blob, want = [], []
    for b in beams:
        ins = np.stack([np.asarray(v, F) for v in _beam_inputs(b)], axis=1)
        fm = fr.beam_eval(*_beam_inputs(b))[0]
        for row, m in zip(ins, fm):
            blob.append(np.array([1], "<u4").tobytes() + row.astype("<f4").tobytes())
            want.append("b %08x" % int(np.array([m], F).view(np.uint32)[0]))
    for b in bufs:
        c = b.metadata.view("<f4")
        ecoef, friction = (F(c[16]) + F(1.0)) / F(2.0), F(c[17])
        for subticks in (64, 60):
            inv_dt2, dt2 = fr.inv_dt2_of(subticks)
            rows = fr.forces_ref(b, subticks=subticks)[0]
            idx = b.mapping[:b.particle_count].astype(int)
            for s, rec in enumerate(fr.partner_records(b)):
                blob.append(np.array([2, len(rec)], "<u4").tobytes() + np.array([20.0, friction, ecoef, inv_dt2, dt2], "<f4").tobytes() + rec.astype("<f4").tobytes())
                r = rows[idx[s]]
                want.append("c %08x %08x %08x %08x %08x %d" % (*[int(x) for x in np.ascontiguousarray(r[2:7]).view(np.uint32)], int(r[7])))
    return b"".join(blob), want


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_header_equals_the_restatement_under_sanitizers(sb, tmp_path, san):
    target = os.path.join("hostcheck_build", "batch_forces_check_" + san)
    p = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    blob, want = _records(sb)
    path = str(tmp_path / "records.bin")
    with open(path, "wb") as f:
        f.write(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(CSRC, target), path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want) > 400
    bad = [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]          # exact, NaN words included: both sides are this CPU's
    assert not bad, bad[:5]
