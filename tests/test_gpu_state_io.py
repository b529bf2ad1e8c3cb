"""The state in device memory (sb_read_state_device / sb_write_particles_device): the export is, byte for byte, what
sb_load_buffers reads back at the same point of the stream, on every schedule, after delete passes and re-uploads; reading changes
nothing; importing what was just exported changes nothing; an import equals the same edit made on the host and uploaded, against the
oracle; torch's stream is ordered against the engine's without an explicit sync.  All comparisons are bit for bit."""
import numpy as np
import pytest

from test_gpu_parity import ATOMIC, GRID, OFF, TILED, assert_same
from test_gpu_reupload import breaking_lattice, moved, without

pytestmark = pytest.mark.gpu

SENT = 0x7FBADBAD    # a NaN payload no step produces: rows the export must not write keep it
SENT_B = 0xA5        # ... and the same for beam_alive
FIELDS = ("target_length", "last_length", "strain", "stress")


def engine(sb, buf, bounds, **kw):
    eng = sb.Engine(bounds_size=bounds, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, **kw)
    eng.write_buffers(buf)
    return eng


def sentinel_tensors(eng):
    import torch
    dev = torch.device("cuda", eng.device)
    p = torch.full((eng.max_particles, 6), SENT, dtype=torch.int32, device=dev).view(torch.float32)
    b = torch.full((eng.max_beams, 4), SENT, dtype=torch.int32, device=dev).view(torch.float32)
    a = torch.full((eng.max_beams,), SENT_B, dtype=torch.uint8, device=dev)
    return p, b, a


def u4(t):
    import torch
    return t.view(torch.int32).cpu().numpy().view("<u4")


def check_export(eng, upload, what):
    """read_state_device == sb_load_buffers now, on sentinel-filled outputs; `upload` = the buffers of the latest upload.  Returns
    load_buffers' state."""
    tp, tb, ta = sentinel_tensors(eng)
    eng.read_state_device(tp, tb, ta)
    gp, gb, ga = u4(tp), u4(tb), ta.cpu().numpy()   # (torch's stream waits for the export: no sync)
    tpl = upload.copy()
    tpl.particles.view("<u4")[:] = SENT
    state = eng.load_buffers(tpl)
    maxP, maxB = upload.max_particles, upload.max_beams
    bad = np.nonzero((gp != state.particles.view("<u4")).any(axis=1))[0]
    assert bad.size == 0, "%s: %d particle rows differ, first %d: %s vs %s" % (
        what, bad.size, bad[0], gp[bad[0]], state.particles.view("<u4")[bad[0]])
    idx = upload.mapping[maxP:maxP + upload.beam_count].astype(np.int64)
    exp_b = np.full((maxB, 4), SENT, dtype="<u4")
    exp_b[idx] = np.stack([state.beams[f] for f in FIELDS], axis=1).astype("<f4").view("<u4")[idx]
    assert np.array_equal(gb, exp_b), "%s: beam rows differ at %s" % (what, np.nonzero((gb != exp_b).any(axis=1))[0][:8])
    exp_a = np.full(maxB, SENT_B, dtype=np.uint8)
    exp_a[idx] = 0
    exp_a[state.mapping[maxP:maxP + state.beam_count].astype(np.int64)] = 1
    assert np.array_equal(ga, exp_a), "%s: beam_alive differs at %s" % (what, np.nonzero(ga != exp_a)[0][:8])
    return state


def round_trip(eng):
    """export, then import the very same tensor"""
    t = eng.state_tensors()
    eng.write_particles_device(t["particles"])


def final(eng, upload):
    return eng.load_buffers(upload.copy()), eng.counts(), eng.info("substeps_done")


def assert_same_run(a, b, what):
    assert_same(a[0], b[0], what)
    assert a[1:] == b[1:], "%s: counts / substeps_done %s vs %s" % (what, a[1:], b[1:])


def quiet_lattice(sb):
    return sb.scenes.lattice_buffers(128, 96, d=30.0, origin=(300.0, 900.0), jitter=1.0, layout=2, velocity=(0.4, -1.0))


SCHEDULES = [
    ("atomic", OFF, ATOMIC, {}),
    ("atomic, grid", GRID, ATOMIC, {}),
    ("tiled, one substep per launch", OFF, TILED, {"block_substeps": 1}),
    ("blocked", OFF, TILED, {}),
    ("tiled, grid", GRID, TILED, {"tile_particles": 256}),
]
CASES = [pytest.param(lay, *s, id="%s-v%d" % (s[0], lay)) for s in SCHEDULES for lay in (1, 2)]


def three_runs(sb, buf, bounds, kw, what, breaks=True):
    """The same run on three engines: N does nothing else, R exports (checked against sb_load_buffers) after every frame and
    mid-frame, I round-trips its particles at a frame boundary and mid-frame.  All three must end bit-identical."""
    engs = {k: engine(sb, buf, bounds, **kw) for k in "NRI"}
    for f in range(3):                   # yields, breaks, delete passes
        for e in engs.values():
            e.frame()
        check_export(engs["R"], buf, "%s, frame %d" % (what, f + 1))
        if f == 1:
            round_trip(engs["I"])
    for e in engs.values():
        e.step(5)                        # mid-frame: break flags pending, strain / stress of a partial call
    check_export(engs["R"], buf, what + ", 5 more substeps")
    round_trip(engs["I"])
    for _ in range(3):
        for e in engs.values():
            e.frame()
    check_export(engs["R"], buf, what + ", 3 frames after")
    out = {k: final(e, buf) for k, e in engs.items()}
    if breaks:
        assert out["N"][1][1] < buf.beam_count, "beams must have broken"
    info = {k: engs["R"].info(k) for k in ("hybrid_launches", "grid_builds")}
    for e in engs.values():
        e.destroy()
    assert_same_run(out["R"], out["N"], what + ": reading changed the run")
    assert_same_run(out["I"], out["N"], what + ": importing what was exported changed the run")
    return info


@pytest.mark.parametrize("layout,what,mode,path,kw", CASES)
def test_every_schedule(sb, layout, what, mode, path, kw):
    """checks 1, 3 and 4 of the issue on every schedule of test_gpu_render.py::test_every_schedule, layouts v1 and v2"""
    buf = breaking_lattice(sb, layout=layout)
    three_runs(sb, buf, 4000.0, dict(collision_mode=mode, path=path, **kw), what)


def test_hybrid_quiet_lattice(sb):
    info = three_runs(sb, quiet_lattice(sb), 6000.0, dict(collision_mode=GRID), "hybrid", breaks=False)
    assert info["hybrid_launches"] > 0, info


def test_config3_pile(sb):
    buf, bounds = sb.scenes.config3_buffers(65536)
    three_runs(sb, buf, bounds, dict(collision_mode=GRID), "pile", breaks=False)


@pytest.mark.parametrize("layout", [1, 2])
def test_tables_follow_uploads(sb, layout):
    """Plan-keeping re-upload, an upload that cut beams, a shuffled mapping: the export follows every upload."""
    from test_render_ref_cpu import shuffled
    first = breaking_lattice(sb, layout=layout)
    eng = engine(sb, first, 4000.0, collision_mode=GRID)
    eng.frame()
    check_export(eng, first, "first")
    second = moved(first, 7)
    eng.write_buffers(second)
    assert eng.info("uploads_kept") == 1
    check_export(eng, second, "kept plan, before a step")
    eng.frame()
    check_export(eng, second, "kept plan")
    cut = without(moved(first, 8), np.random.default_rng(11).random(first.beam_count) >= 0.01)
    eng.write_buffers(cut)
    assert eng.info("uploads_edited") >= 1
    check_export(eng, cut, "cut, before a step")
    for _ in range(2):
        eng.frame()
        check_export(eng, cut, "cut")
    eng.step(5)
    check_export(eng, cut, "cut, mid-frame")
    state = eng.load_buffers(cut.copy())
    sh = shuffled(state, 4)
    eng.write_buffers(sh)
    check_export(eng, sh, "shuffled")
    eng.frame()
    check_export(eng, sh, "shuffled, a frame")
    eng.destroy()


def corner_block(upload, d, n=10):
    """data indices of the n x n lattice corner with the smallest x and y (at upload)"""
    P = upload.particle_count
    rows = upload.mapping[:P].astype(np.int64)
    xy = upload.particles[rows, :2].astype(np.float64)
    lo = xy.min(axis=0)
    sel = (xy[:, 0] < lo[0] + (n - 0.5) * d) & (xy[:, 1] < lo[1] + (n - 0.5) * d)
    assert sel.sum() == n * n
    return rows[sel]


@pytest.mark.parametrize("what,mode,path", [("default, hybrid", GRID, 0), ("blocked, collisions off", OFF, TILED),
                                            ("atomic", GRID, ATOMIC)])
def test_import_equals_host_edit(sb, oracle, what, mode, path):
    """Check 5: an edit made with torch on the device and imported == the same edit made in numpy and uploaded to the oracle.
    Against libraries built without the import's hash / hybrid reset, the atomic case fails; without the acceleration flag, the
    hybrid and blocked cases fail.  The hybrid case alone passes without the reset: the shift halves the block's beams, the tracked
    blocked launches measure the motion that follows, go over their budget and are redone behind a fresh hash."""
    import torch
    buf = quiet_lattice(sb)
    eng = engine(sb, buf, 6000.0, collision_mode=mode, path=path)
    ref = oracle.OracleEngine(6000.0, 10.0, 64, 2, mode, threads=16)
    ref.write_buffers(buf)
    for _ in range(3):
        eng.frame()
        ref.frame()
    base = eng.load_buffers(buf.copy())
    assert_same(base, ref.load_buffers(buf.copy()), what + ": before the import")
    P = base.particle_count
    rows = base.mapping[:P].astype(np.int64)
    if mode == GRID and path == 0:
        assert eng.info("hybrid_launches") > 0, "blocked launches must have run before the import"
    if mode == OFF:
        assert not base.particles[rows, 4:6].view("<u4").any(), "accelerations must all be zero before the import"
    # the edit: velocities scaled, the corner block shifted by half a spacing (new contacts), accelerations set (nonzero / -0.0)
    rng = np.random.default_rng(5)
    factor = np.float32(rng.uniform(0.6, 1.4))
    block = corner_block(buf, 30.0)
    acc_rows = rows[rng.permutation(P)[:P // 7]]
    neg0_rows = np.setdiff1d(rows[rng.permutation(P)[:P // 5]], acc_rows)
    acc_val = np.asarray([0.25, -0.75], "<f4")
    edited = base.copy()
    edited.particles[rows, 2:4] *= factor
    edited.particles[block, 0] += np.float32(15.0)
    edited.particles[acc_rows, 4:6] = acc_val
    edited.particles[neg0_rows, 4:6] = np.float32(-0.0)
    t = eng.state_tensors()
    dev = t["particles"].device
    rt, bt, at, nt = (torch.from_numpy(x).to(dev) for x in (rows, block, acc_rows, neg0_rows))
    t["particles"][rt, 2:4] *= torch.tensor(factor, dtype=torch.float32, device=dev)
    t["particles"][bt, 0] += torch.tensor(np.float32(15.0), dtype=torch.float32, device=dev)
    t["particles"][at, 4:6] = torch.from_numpy(acc_val).to(dev)
    t["particles"][nt, 4:6] = -0.0
    eng.write_particles_device(t["particles"])
    imported = eng.load_buffers(base.copy())   # the import, read back before any step
    assert np.array_equal(imported.particles.view("<u4"), edited.particles.view("<u4")), what + ": the import is not the edit"
    ref.write_buffers(edited)
    for _ in range(3):
        eng.frame()
        ref.frame()
    got, exp = eng.load_buffers(edited.copy()), ref.load_buffers(edited.copy())
    assert eng.counts() == (exp.particle_count, exp.beam_count)
    assert_same(got, exp, what + ": 3 frames after the import")
    assert not np.array_equal(got.particles, base.particles)
    eng.destroy()


def test_torch_ordering(sb):
    """Check 6: state_tensors, a torch edit, the import and a frame with no explicit sync == the same edit through the host (both
    read back into copies of the state after the first frame, so that beams removed before the edit read the same)."""
    buf = breaking_lattice(sb)
    out, tpl = [], None
    for device_side in (False, True):
        eng = engine(sb, buf, 4000.0, collision_mode=GRID)
        eng.frame()
        if device_side:
            t = eng.state_tensors()
            t["particles"][:, 2:4] *= 0.5
            eng.write_particles_device(t["particles"])
        else:
            tpl = eng.load_buffers(buf.copy())
            h = tpl.copy()
            h.particles[:, 2:4] *= np.float32(0.5)
            eng.write_buffers(h)
        eng.frame()
        out.append(eng.load_buffers(tpl.copy()))
        eng.destroy()
    assert_same(out[1], out[0], "torch edit vs host edit")


def test_config2_full_size(sb):
    """Check 7: 1 M particles / 3 M beams, v2: the export equals sb_load_buffers; a round trip changes nothing."""
    buf = sb.scenes.lattice_buffers(1000, 1000, d=30.0, origin=(1000.0, 1000.0), jitter=1.0, layout=2)
    runs = []
    for trip in (True, False):
        eng = engine(sb, buf, 32000.0, collision_mode=OFF)
        eng.step(20)
        if trip:
            check_export(eng, buf, "config 2")
            round_trip(eng)
        eng.step(20)
        runs.append(final(eng, buf))
        eng.destroy()
    assert_same_run(runs[0], runs[1], "config 2: importing what was exported changed the run")


def test_errors(sb):
    """Check 8: SB_ERR_STATE before an upload, SB_ERR_UNSUPPORTED with ghost zones, SB_ERR_INVALID for a NULL import source;
    ValueError for a CPU tensor, a wrong dtype, a too small and a non-contiguous tensor."""
    import ctypes
    import torch
    from softbody_webgpu_amd.engine import EngineError
    lib = sb.engine.load_library()
    buf = sb.scenes.default_buffers(2, 256, 512)
    eng = sb.Engine(layout=2, max_particles=256, max_beams=512)
    dev = torch.device("cuda", 0)
    p = torch.zeros((256, 6), dtype=torch.float32, device=dev)
    for call in (lambda: eng.read_state_device(p), lambda: eng.write_particles_device(p), lambda: eng.state_tensors()):
        with pytest.raises(EngineError) as ex:
            call()
        assert ex.value.status == 5   # SB_ERR_STATE
    eng.write_buffers(buf)
    eng.frame()
    assert lib.sb_write_particles_device(eng._h, None) == 1   # SB_ERR_INVALID
    with pytest.raises(EngineError) as ex:
        eng.write_particles_device(0)
    assert ex.value.status == 1
    assert lib.sb_read_state_device(eng._h, None, None, None) == 0
    bad = [torch.zeros((256, 6), dtype=torch.float32),                        # on the CPU
           torch.zeros((256, 6), dtype=torch.float64, device=dev),            # wrong dtype
           torch.zeros((255, 6), dtype=torch.float32, device=dev),            # too small
           torch.zeros((256, 12), dtype=torch.float32, device=dev)[:, ::2]]   # not contiguous
    for x in bad:
        with pytest.raises(ValueError):
            eng.read_state_device(x)
        with pytest.raises(ValueError):
            eng.write_particles_device(x)
    for x in (torch.zeros(512, dtype=torch.uint8), torch.zeros(512, dtype=torch.int8, device=dev),
              torch.zeros(511, dtype=torch.uint8, device=dev)):
        with pytest.raises(ValueError):
            eng.read_state_device(beam_alive=x)
    for x in (torch.zeros((512, 8), dtype=torch.float32, device=dev)[:, :4], torch.zeros((511, 4), dtype=torch.float32, device=dev)):
        with pytest.raises(ValueError):
            eng.read_state_device(beams=x)
    eng.read_state_device(p)   # (the engine is still usable)
    eng.sync()
    eng.destroy()
    # ghost zones configured: not handled
    eng = sb.Engine(layout=2, max_particles=256, max_beams=512, collision_mode=OFF, path=TILED)
    eng.write_buffers(buf)
    eng.halo_configure([0, 1], [2, 3])
    for call in (lambda: eng.read_state_device(p), lambda: eng.write_particles_device(p)):
        with pytest.raises(EngineError) as ex:
            call()
        assert ex.value.status == 6   # SB_ERR_UNSUPPORTED
    assert lib.sb_read_state_device(eng._h, ctypes.c_void_p(p.data_ptr()), None, None) == 6
    eng.destroy()
