"""Engine.checkpoint / Engine.restore (sb_checkpoint_device / sb_restore_device): after a restore every read-back,
report and later step gives the bits the engine gave -- or would have given -- at and after the checkpoint, on every schedule: across
delete passes that removed beams since, from a checkpoint taken mid-frame with break flags pending, under the hybrid, after imports
and after an upload that cut beams.  All comparisons are bit for bit."""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import ATOMIC, GRID, OFF, TILED, assert_same
from test_gpu_reupload import breaking_lattice, moved, without
from test_gpu_state_io import SCHEDULES, assert_same_run, check_export, final, quiet_lattice

pytestmark = pytest.mark.gpu

CASES = [pytest.param(lay, *s, id="%s-v%d" % (s[0], lay)) for s in SCHEDULES for lay in (1, 2)]
ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 5, 6


def engine(sb, buf, bounds, **kw):
    eng = sb.Engine(bounds_size=bounds, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, **kw)
    eng.write_buffers(buf)
    return eng


def run_on(eng):
    for _ in range(3):
        eng.frame()
    eng.step(5)


def rewind(sb, buf, bounds, kw, what, breaks=True, probe=None):
    """Two engines: N runs straight, C rewinds.  Both run 2 frames; C checkpoints, runs 3 frames + 5 substeps (recorded), restores,
    runs the same again: it must equal the recording, and so must N; then both run 2 more frames and must be equal.  probe(C) is
    called at the checkpoint, before the restore and at the end; its values are returned."""
    N, C = engine(sb, buf, bounds, **kw), engine(sb, buf, bounds, **kw)
    for e in (N, C):
        e.frame()
        e.frame()
    seen = []
    C.checkpoint()
    at_ck = (C.counts(), C.info("substeps_done"))
    if probe:
        seen.append(probe(C))
    run_on(C)
    first = final(C, buf)
    if probe:
        seen.append(probe(C))
    if breaks:
        assert first[1][1] < at_ck[0][1], what + ": beams must break between the checkpoint and the restore"
    C.restore()
    assert (C.counts(), C.info("substeps_done")) == at_ck, what + ": counts / substeps_done right after the restore"
    run_on(C)
    assert_same_run(final(C, buf), first, what + ": the run after the restore is not the run after the checkpoint")
    run_on(N)
    assert_same_run(final(N, buf), first, what + ": the straight run")
    for e in (N, C):
        e.frame()
        e.frame()
    out = final(C, buf), final(N, buf)
    if probe:
        seen.append(probe(C))
    assert C.info("checkpoints") == 1 and C.info("restores") == 1 and C.info("checkpoint_bytes") > 0
    assert N.info("checkpoints") == 0 and N.info("checkpoint_bytes") == 0
    N.destroy()
    C.destroy()
    assert_same_run(out[0], out[1], what + ": 2 frames later")
    return seen


@pytest.mark.parametrize("layout,what,mode,path,kw", CASES)
def test_every_schedule(sb, layout, what, mode, path, kw):
    """1: every schedule x layouts v1 / v2; the restore crosses delete passes that removed beams."""
    rewind(sb, breaking_lattice(sb, layout=layout), 4000.0, dict(collision_mode=mode, path=path, **kw), what)


@pytest.mark.parametrize("at", [5, -5], ids=["5-in", "5-before-the-end"])
@pytest.mark.parametrize("what,mode,path,kw", SCHEDULES, ids=[s[0] for s in SCHEDULES])
def test_mid_frame_checkpoint(sb, what, mode, path, kw, at):
    """2: a checkpoint 5 substeps into (and, so that break flags are pending for certain, 5 substeps before the end of) the first
    frame whose delete pass removes something; C runs on through that pass and one more frame, restores, finishes the frame: N's
    state at that frame boundary."""
    buf = breaking_lattice(sb)
    kw = dict(collision_mode=mode, path=path, **kw)
    N = engine(sb, buf, 4000.0, **kw)
    k, boundary = None, None
    for f in range(8):
        before = N.counts()[1]
        N.frame()
        if N.counts()[1] < before:
            k, boundary = f, final(N, buf)
            break
    N.destroy()
    assert k is not None, "no delete pass removed anything in 8 frames"
    C = engine(sb, buf, 4000.0, **kw)
    for _ in range(k):
        C.frame()
    at = at % C.subticks
    C.step(at)
    flagged = C.info("beams_flagged")
    print("%s: frame %d, %d substeps in, break flags pending at the checkpoint: %d" % (what, k, at, flagged))
    assert at == 5 or flagged > 0, "no break flag pending %d substeps into the frame" % at
    C.checkpoint()
    mid = final(C, buf)
    C.step(C.subticks - at)
    C.delete_pass()
    C.frame()
    C.restore()
    check_export(C, buf, what + ": right after the restore")
    assert_same_run(final(C, buf), mid, what + ": the state right after the restore")
    C.step(C.subticks - at)
    C.delete_pass()
    got = final(C, buf)
    C.destroy()
    assert_same_run(got, boundary, what + ": the frame finished after the restore")


def test_hybrid_quiet_lattice(sb):
    """3: the blocked plan beside the tiled layout, and the forced hash build: blocked launches on both sides of the restore."""
    h = rewind(sb, quiet_lattice(sb), 6000.0, dict(collision_mode=GRID), "hybrid", breaks=False, probe=lambda e: e.info("hybrid_launches"))
    assert h[0] < h[1] < h[2], h


def test_config3_pile(sb):
    buf, bounds = sb.scenes.config3_buffers(65536)
    rewind(sb, buf, bounds, dict(collision_mode=GRID), "pile", breaks=False)


def reports(eng):
    out = []
    for r in (eng.summary_host(), eng.bodies_host(), eng.contacts_host(), eng.body_summary_host()):
        out += [np.ascontiguousarray(x).tobytes() for x in r]
    out.append(eng.render(64).tobytes())
    return out


@pytest.mark.parametrize("what,mode,path,kw", [SCHEDULES[3], ("default", GRID, 0, {})], ids=["blocked", "default"])
def test_reports_follow(sb, what, mode, path, kw):
    """4: summary, bodies, contacts, body_summary and the picture at the checkpoint == after the run-on and the restore."""
    buf = breaking_lattice(sb)
    eng = engine(sb, buf, 4000.0, collision_mode=mode, path=path, **kw)
    eng.frame()
    eng.frame()
    eng.checkpoint()
    at_ck = reports(eng)
    run_on(eng)
    later = reports(eng)
    assert later != at_ck, "the run-on must change the reports"
    eng.restore()
    back = reports(eng)
    eng.destroy()
    names = ["summary row", "summary counts", "bodies labels", "bodies sizes", "bodies counts", "contacts touch", "contacts counts",
             "contacts pairs", "body_summary rows", "body_summary counts", "body_summary rank", "render"]
    for n, a, b in zip(names, at_ck, back):
        assert a == b, "%s: %s differs after the restore" % (what, n)


@pytest.mark.parametrize("what,mode,path,kw", [SCHEDULES[3], SCHEDULES[4], ("default", GRID, 0, {})], ids=["blocked", "tiled-grid", "default"])
def test_restore_undoes_imports(sb, what, mode, path, kw):
    """5: checkpoint, particle and beam imports, a frame, restore == an engine that never imported."""
    import torch
    buf = breaking_lattice(sb)
    A, B = (engine(sb, buf, 4000.0, collision_mode=mode, path=path, **kw) for _ in range(2))
    for e in (A, B):
        e.frame()
        e.frame()
    A.checkpoint()
    dev = torch.device("cuda", A.device)
    A.write_particles_device(torch.from_numpy(moved(buf, 3).particles.copy()).to(dev))
    t = A.state_tensors()
    t["beams"][:, 0] *= 0.9
    A.write_beams_device(t["beams"], target_length=True, last_length=True)
    A.frame()
    assert A.load_buffers(buf.copy()).particles.tobytes() != B.load_buffers(buf.copy()).particles.tobytes()
    A.restore()
    for e in (A, B):
        e.frame()
        e.step(5)
    out = final(A, buf), final(B, buf)
    A.destroy()
    B.destroy()
    assert_same_run(out[0], out[1], what + ": the imports survived the restore")


@pytest.mark.parametrize("what,mode,path,kw", [SCHEDULES[0], SCHEDULES[3], ("default", GRID, 0, {})], ids=["atomic", "blocked", "default"])
def test_after_an_upload_that_cut_beams(sb, what, mode, path, kw):
    """6: a checkpoint behind the upload's generation-1 delete pass; frames that break more; counts, mapping and state read back
    as at the checkpoint, and the run goes on as that of an engine that never rewound."""
    first = breaking_lattice(sb)
    cut = without(moved(first, 8), np.random.default_rng(11).random(first.beam_count) >= 0.01)
    engs = [engine(sb, first, 4000.0, collision_mode=mode, path=path, **kw) for _ in range(2)]
    for e in engs:
        e.frame()
        e.write_buffers(cut)
        assert e.info("uploads_edited") == 1
        e.frame()
    C, N = engs
    C.checkpoint()
    at_ck = final(C, cut)
    run_on(C)
    assert C.counts()[1] < at_ck[1][1], "beams must break after the checkpoint"
    C.restore()
    assert_same_run(final(C, cut), at_ck, what + ": read back after the restore")
    check_export(C, cut, what + ": export after the restore")
    for e in engs:
        run_on(e)
    out = final(C, cut), final(N, cut)
    for e in engs:
        e.destroy()
    assert_same_run(out[0], out[1], what + ": the run after the restore")


def status_of(call):
    from softbody_webgpu_amd.engine import EngineError
    with pytest.raises(EngineError) as ex:
        call()
    return ex.value.status


def test_lifecycle(sb):
    """7: no checkpoint -> SB_ERR_STATE; every upload drops it; a second checkpoint replaces the first; restores are idempotent; ghost
    zones -> SB_ERR_UNSUPPORTED; argument errors -> SB_ERR_INVALID."""
    import torch
    lib = sb.engine.load_library()
    vp = ctypes.c_void_p
    buf = breaking_lattice(sb)
    dev = torch.device("cuda", 0)
    rows = torch.zeros((buf.max_beams, 4), dtype=torch.float32, device=dev)
    eng = sb.Engine(bounds_size=4000.0, layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=OFF)
    for call in (eng.checkpoint, eng.restore, lambda: eng.write_beams_device(rows)):
        assert status_of(call) == ERR_STATE     # before an upload
    eng.write_buffers(buf)
    assert status_of(eng.restore) == ERR_STATE and eng.info("checkpoint_bytes") == 0
    eng.frame()
    eng.checkpoint()
    nbytes = eng.info("checkpoint_bytes")
    assert nbytes > 0
    one = final(eng, buf)
    eng.frame()
    eng.checkpoint()                            # replaces the first
    assert eng.info("checkpoint_bytes") == nbytes and eng.info("checkpoints") == 2
    two = final(eng, buf)
    run_on(eng)
    eng.restore()
    assert_same_run(final(eng, buf), two, "the second checkpoint")
    eng.restore()                               # idempotent
    assert_same_run(final(eng, buf), two, "a second restore")
    assert two[2] != one[2] and eng.info("restores") == 2
    eng.write_buffers(moved(buf, 2))            # plan-keeping: the checkpoint is gone
    assert eng.info("uploads_kept") == 1
    assert status_of(eng.restore) == ERR_STATE and eng.info("checkpoint_bytes") == 0
    # argument errors
    assert lib.sb_write_beams_device(eng._h, None, 1) == ERR_INVALID
    assert lib.sb_write_beams_device(eng._h, vp(rows.data_ptr() + 8), 1) == ERR_INVALID     # not 16-byte aligned
    assert lib.sb_write_beams_device(eng._h, vp(rows.data_ptr()), 0) == ERR_INVALID
    assert lib.sb_write_beams_device(eng._h, vp(rows.data_ptr()), 4) == ERR_INVALID
    assert lib.sb_write_beams_device(eng._h, vp(rows.data_ptr()), 7) == ERR_INVALID
    assert lib.sb_checkpoint_device(None) == ERR_INVALID and lib.sb_restore_device(None) == ERR_INVALID
    with pytest.raises(ValueError):
        eng.write_beams_device(rows, target_length=False, last_length=False)
    for bad in (torch.zeros((buf.max_beams, 4), dtype=torch.float32), torch.zeros((buf.max_beams, 4), dtype=torch.float64, device=dev),
                torch.zeros((buf.max_beams - 1, 4), dtype=torch.float32, device=dev)):
        with pytest.raises(ValueError):
            eng.write_beams_device(bad)
    eng.checkpoint()
    eng.destroy()                               # (with a checkpoint held)
    # ghost zones configured: none of the three calls handles ranks; configuring drops the checkpoint
    small = sb.scenes.default_buffers(2, 256, 512)
    eng = sb.Engine(layout=2, max_particles=256, max_beams=512, collision_mode=OFF, path=TILED)
    eng.write_buffers(small)
    eng.checkpoint()
    eng.halo_configure([0, 1], [2, 3])
    assert eng.info("checkpoint_bytes") == 0
    srows = torch.zeros((512, 4), dtype=torch.float32, device=dev)
    for call in (eng.checkpoint, eng.restore, lambda: eng.write_beams_device(srows)):
        assert status_of(call) == ERR_UNSUPPORTED
    eng.destroy()
