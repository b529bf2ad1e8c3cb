"""Beam import, particle import, checkpoint and restore on EACH half of the engine's double buffers.
The blocked layout keeps target, last length and the plastic flags in two halves and flips `bk.cur` with every launch, the particle
buffers and the acceleration flags flip with `e->cur`; which write of an import and which copy of a restore matters depends on the
half that is current at the call.  step(1) is exactly one launch, so a frame followed by one or two step(1) reaches either half for
certain; every test asserts the half it is on through info "state_half" / "beam_state_half".  tests/test_state_io_model_cpu.py runs
these scenarios over a model of the store and lists, per omitted write, which of them notices.  All comparisons are bit for bit."""
import numpy as np
import pytest

from test_gpu_beam_import import NAN, NEG_ZERO, beam_rows, device_rows, far_block, the_edit
from test_gpu_parity import OFF, TILED, assert_same
from test_gpu_reupload import breaking_lattice
from test_gpu_state_io import SCHEDULES, check_export, corner_block, engine, quiet_lattice

pytestmark = pytest.mark.gpu

BLOCKED = dict(collision_mode=OFF, path=TILED)
HALVES = pytest.mark.parametrize("h", [0, 1], ids=["half0", "half1"])


def halves(eng):
    return eng.info("state_half"), eng.info("beam_state_half")


def reach(eng, h, blocked, followers=()):
    """one step(1), and one more if that is not half h; `followers` make the same calls.  Asserts the half."""
    n = 1
    eng.step(1)
    if eng.info("state_half") != h:
        eng.step(1)
        n = 2
    for f in followers:
        for _ in range(n):
            f.step(1)
    for e in (eng,) + tuple(followers):
        assert halves(e) == (h, h if blocked else 0), "half %d not reached: %s" % (h, halves(e))
    return n


def snap(eng, tpl, substeps=True, flags=True):
    """the read-back, the counts, the two flag counts (`flags`: engines without a hybrid plan, whose rows a restore resets) and the
    substep count (`substeps`: not against an engine that was uploaded later)"""
    return (eng.load_buffers(tpl.copy()), eng.counts(), eng.info("plastic_tiles") if flags else None,
            eng.info("acc_dirty_tiles") if flags else None, eng.info("substeps_done") if substeps else None)


def same(a, b, what, acc=True):
    """acc=False: right after an upload, which raises the acceleration flag of every tile (reset_run_state, sb_api.hip); the first
    launch recomputes the row"""
    assert_same(a[0], b[0], what)
    assert a[1] == b[1], "%s: counts %s vs %s" % (what, a[1], b[1])
    assert a[2] == b[2], "%s: plastic_tiles %s vs %s" % (what, a[2], b[2])
    assert not acc or a[3] == b[3], "%s: acc_dirty_tiles %s vs %s" % (what, a[3], b[3])
    assert a[4] == b[4], "%s: substeps_done %s vs %s" % (what, a[4], b[4])


def blocked_quiet(sb, buf):
    eng = engine(sb, buf, 6000.0, **BLOCKED)
    assert eng.info("substeps_per_launch") > 1 and eng.info("tiles") >= 4 and eng.info("plastic_tiles") == 0, "no tile may be flagged"
    return eng


def edit_a(upload, base):
    """test_gpu_beam_import.the_edit (a corner block's targets to 0.8 rest length, the far block's last lengths x 1.1, a NaN target,
    a -0.0 last length) and one target changed by one bit, far from both blocks"""
    edited, t_rows, l_rows = the_edit(upload, base)
    free = np.setdiff1d(beam_rows(base), np.concatenate([t_rows, l_rows]))
    one = free[free.size // 4]
    assert edited.beams["target_length"].view("<u4")[one] == base.beams["target_length"].view("<u4")[one]
    edited.beams["target_length"].view("<u4")[one] += 1
    return edited


def step_and_compare(A, B, tpl, what, steps, frames, substeps=False):
    for i in range(steps):
        for e in (A, B):
            e.step(1)
        same(snap(A, tpl, substeps), snap(B, tpl, substeps), "%s: step(1) number %d after" % (what, i + 1))
    for e in (A, B):
        for _ in range(frames):
            e.frame()
    out = snap(A, tpl, substeps), snap(B, tpl, substeps)
    same(out[0], out[1], "%s: %d frames after" % (what, frames))
    return out[0]


# ---- a. blocked beam import on each half

@HALVES
def test_blocked_import(sb, oracle, h):
    """a: the edit imported on half h == the edited buffers uploaded, right after the import, after each of three step(1) -- a stale
    half shows on the first or the second launch -- and two frames later, where both equal the oracle."""
    what = "blocked import on half %d" % h
    buf = quiet_lattice(sb)
    A = blocked_quiet(sb, buf)
    A.frame()
    reach(A, h, True)
    assert A.info("plastic_tiles") == 0
    base = A.load_buffers(buf.copy())
    edited = edit_a(buf, base)
    A.write_beams_device(device_rows(A, edited), target_length=True, last_length=True)
    assert halves(A) == (h, h)
    imported = A.load_buffers(base.copy())
    assert imported.beams.tobytes() == edited.beams.tobytes(), what + ": the read-back is not the edit"
    assert imported.particles.tobytes() == base.particles.tobytes()
    check_export(A, buf, what)
    B = blocked_quiet_edited(sb, edited)
    same(snap(A, edited, False), snap(B, edited, False), what + ": right after", acc=False)
    assert A.info("plastic_tiles") >= 2, "the block and, far from it, the one bit and the NaN raise flags"
    got = step_and_compare(A, B, edited, what, 3, 2)
    A.destroy()
    B.destroy()
    ref = oracle.OracleEngine(6000.0, 10.0, 64, edited.layout, OFF, threads=16)
    ref.write_buffers(edited)
    ref.step(3)
    ref.frame()
    ref.frame()
    assert_same(got[0], ref.load_buffers(edited.copy()), what + ": against the oracle")
    assert not np.array_equal(got[0].particles[corner_block(buf, 30.0)], base.particles[corner_block(buf, 30.0)])


def blocked_quiet_edited(sb, edited):
    eng = engine(sb, edited, 6000.0, **BLOCKED)
    assert eng.info("substeps_per_launch") > 1 and halves(eng) == (0, 0)
    return eng


@HALVES
def test_flag_rule_is_on_words(sb, h):
    """a, for the flag rule alone (the model's a-words script): a beam uploaded with a NaN as rest length and the same NaN as target
    (no flag: the words are equal) gets that NaN imported again.  No flag may be raised, as the upload's memcmp raises none -- != on
    floats would raise one.  (A NaN strain passes no comparison: the beam neither yields nor breaks; the NaN it spreads through the
    particles is the same bits on both engines.)"""
    what = "a NaN target over the same NaN rest length, on half %d" % h
    buf = quiet_lattice(sb)
    rows = beam_rows(buf)
    odd = rows[rows.size // 2]
    for f in ("length", "target_length"):
        buf.beams[f].view("<u4")[odd] = NAN
    A = blocked_quiet(sb, buf)
    reach(A, h, True)
    assert A.info("plastic_tiles") == 0 and A.counts()[1] == buf.beam_count
    base = A.load_buffers(buf.copy())
    edited = base.copy()
    assert edited.beams["target_length"].view("<u4")[odd] == NAN
    edited.beams["target_length"].view("<u4")[rows[rows.size // 3]] += 1     # (and one bit elsewhere: exactly one flag)
    A.write_beams_device(device_rows(A, edited), target_length=True, last_length=False)
    B = blocked_quiet_edited(sb, edited)
    assert A.info("plastic_tiles") == 1 and B.info("plastic_tiles") == 1, what
    same(snap(A, edited, False), snap(B, edited, False), what + ": right after", acc=False)
    step_and_compare(A, B, edited, what, 3, 0)
    A.destroy()
    B.destroy()


# ---- b. field masks on each half

@HALVES
@pytest.mark.parametrize("field", ["target_length", "last_length"])
def test_field_mask(sb, field, h):
    """b: one field of the edit imported on half h == that field alone edited on the host and uploaded, over three step(1)."""
    what = "%s only, on half %d" % (field, h)
    buf = quiet_lattice(sb)
    A = blocked_quiet(sb, buf)
    A.frame()
    reach(A, h, True)
    base = A.load_buffers(buf.copy())
    edited = edit_a(buf, base)
    only = base.copy()
    only.beams[field] = edited.beams[field]
    assert only.beams.tobytes() not in (base.beams.tobytes(), edited.beams.tobytes())
    A.write_beams_device(device_rows(A, edited), target_length=field == "target_length", last_length=field == "last_length")
    assert A.load_buffers(base.copy()).beams.tobytes() == only.beams.tobytes(), what + ": the read-back"
    B = blocked_quiet_edited(sb, only)
    same(snap(A, only, False), snap(B, only, False), what + ": right after", acc=False)
    step_and_compare(A, B, only, what, 3, 0)
    A.destroy()
    B.destroy()


# ---- c. checkpoint half x restore half

# (the 1 200-particle scene makes two tiles of the default size on the single-substep tiling: 256-particle tiles there too)
C_SCHEDULES = [SCHEDULES[3], SCHEDULES[2][:3] + (dict(SCHEDULES[2][3], tile_particles=256),), SCHEDULES[0], SCHEDULES[4]]


@pytest.mark.parametrize("a,b", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["ck0-re0", "ck0-re1", "ck1-re0", "ck1-re1"])
@pytest.mark.parametrize("what,mode,path,kw", C_SCHEDULES, ids=[s[0] for s in C_SCHEDULES])
def test_checkpoint_half_restore_half(sb, what, mode, path, kw, a, b):
    """c: checkpoint on half a; three step(1) and three frames (recorded), 5 substeps, beams break; on half b the restore.  The halves,
    the counts, substeps_done and the read-back are the checkpoint's; the rerun equals the recording and an engine that never
    rewound, after each step(1) and after the frames."""
    blocked = what == "blocked"
    what = "%s, checkpoint on half %d, restore on half %d" % (what, a, b)
    buf = breaking_lattice(sb)
    N, C = (engine(sb, buf, 4000.0, collision_mode=mode, path=path, **kw) for _ in range(2))
    if path == TILED:
        assert C.info("tiles") >= 4
    assert (C.info("substeps_per_launch") > 1) == blocked
    for e in (N, C):
        e.frame()
    reach(C, a, blocked, followers=(N,))
    flags = mode == OFF and path == TILED

    def snap_c(e):
        return snap(e, buf, flags=flags)

    C.checkpoint()
    at_ck = snap_c(C)
    check_export(C, buf, what + ": at the checkpoint")

    def run(e, record):
        for _ in range(3):
            e.step(1)
            record.append(snap_c(e))
        for _ in range(3):
            e.frame()
        record.append(snap_c(e))

    first, again, straight = [], [], []
    run(C, first)
    C.step(5)
    reach(C, b, blocked)
    assert C.counts()[1] < at_ck[1][1], what + ": beams must break between the checkpoint and the restore"
    C.restore()
    assert halves(C) == (a, a if blocked else 0), what + ": the halves right after the restore"
    assert (C.counts(), C.info("substeps_done")) == (at_ck[1], at_ck[4]), what + ": counts / substeps_done right after the restore"
    same(snap_c(C), at_ck, what + ": the read-back right after the restore")
    check_export(C, buf, what + ": right after the restore")
    run(C, again)
    run(N, straight)
    N.destroy()
    C.destroy()
    labels = ["step(1) number %d" % i for i in (1, 2, 3)] + ["three frames"]
    for l, f, g, s in zip(labels, first, again, straight):
        same(g, f, "%s: the rerun is not the recording, %s after" % (what, l))
        same(s, f, "%s: the straight run is not the recording, %s after" % (what, l))


# ---- d. a restore undoes an import made on the other half

@HALVES
def test_restore_undoes_import_on_other_half(sb, h):
    """d: checkpoint on half h, one launch, targets and last lengths imported (on the other half), a frame, the restore == an engine
    that never imported: after each of three step(1) and after two frames, plastic_tiles included."""
    what = "checkpoint on half %d, import on half %d" % (h, h ^ 1)
    buf = breaking_lattice(sb)
    A, B = (engine(sb, buf, 4000.0, **BLOCKED) for _ in range(2))
    assert A.info("substeps_per_launch") > 1 and A.info("tiles") >= 4
    for e in (A, B):
        e.frame()
    reach(A, h, True, followers=(B,))
    A.checkpoint()
    A.step(1)
    assert halves(A) == (h ^ 1, h ^ 1)
    t = A.state_tensors()
    t["beams"][:, 0] *= 0.9
    t["beams"][:, 1] *= 1.05
    A.write_beams_device(t["beams"], target_length=True, last_length=True)
    A.frame()
    assert A.load_buffers(buf.copy()).particles.tobytes() != B.load_buffers(buf.copy()).particles.tobytes()
    A.restore()
    assert halves(A) == (h, h)
    same(snap(A, buf), snap(B, buf), what + ": right after the restore")
    step_and_compare(A, B, buf, what, 3, 2, substeps=True)
    A.destroy()
    B.destroy()


# ---- e. particle import on each half

@HALVES
@pytest.mark.parametrize("what,mode,path,kw", [SCHEDULES[3], SCHEDULES[2]], ids=["blocked", "tiled-1"])
def test_particle_import(sb, what, mode, path, kw, h):
    """e: on half h, nonzero accelerations imported into one corner block, exact zeros into the other, which held nonzero ones, and one
    -0.0 in between == the same edit uploaded: the buffers right after the import, buffers and acc_dirty_tiles after each of two
    step(1) and after a frame.
    acc_dirty_tiles right after the import cannot be compared with the uploaded engine's: an upload raises the flag of EVERY tile of
    buffer 0 (reset_run_state, sb_api.hip: "buffer A holds whatever accelerations were uploaded"), and an import raises flags and
    never lowers one.  Asserted there instead: the upload's count is the number of tiles, the import's is at least the two tiles that
    hold nonzero bits.  From the first launch on both rows are recomputed from the accelerations and must be equal."""
    blocked = what == "blocked"
    what = "particle import, %s, half %d" % (what, h)
    buf = quiet_lattice(sb)
    A = engine(sb, buf, 6000.0, collision_mode=mode, path=path, **kw)
    tiles = A.info("tiles")
    assert tiles >= 4 and (A.info("substeps_per_launch") > 1) == blocked
    A.frame()
    reach(A, h, blocked)
    assert A.info("acc_dirty_tiles") == 0, "accelerations must all be zero before the imports"
    import torch
    dev = torch.device("cuda", A.device)
    near, far = corner_block(buf, 30.0), far_block(buf, 30.0)
    rows = buf.mapping[:buf.particle_count].astype(np.int64)
    mid = np.setdiff1d(rows, np.concatenate([near, far]))
    mid = mid[mid.size // 2]
    before = A.load_buffers(buf.copy())
    before.particles[far, 4:6] = np.asarray([-0.5, 0.125], "<f4")
    A.write_particles_device(torch.from_numpy(before.particles.copy()).to(dev))     # the far block now holds nonzero accelerations
    assert 1 <= A.info("acc_dirty_tiles") < tiles and halves(A) == (h, h if blocked else 0)
    edited = A.load_buffers(buf.copy())
    assert edited.particles[far, 4:6].view("<u4").all()
    edited.particles[near, 4:6] = np.asarray([0.25, -0.75], "<f4")
    edited.particles[far, 4:6] = 0.0
    edited.particles.view("<u4")[mid, 4] = NEG_ZERO
    A.write_particles_device(torch.from_numpy(edited.particles.copy()).to(dev))
    assert halves(A) == (h, h if blocked else 0)
    assert A.load_buffers(buf.copy()).particles.tobytes() == edited.particles.tobytes(), what + ": the read-back is not the edit"
    B = engine(sb, edited, 6000.0, collision_mode=mode, path=path, **kw)
    a0, b0 = snap(A, edited, False), snap(B, edited, False)
    same(a0, b0, what + ": right after", acc=False)
    assert b0[3] == tiles and 2 <= a0[3] < tiles, "acc_dirty_tiles right after: import %d, upload %d of %d tiles" % (a0[3], b0[3], tiles)
    step_and_compare(A, B, edited, what, 2, 1)
    A.destroy()
    B.destroy()
