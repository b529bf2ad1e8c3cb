"""Engine.forces() (sb_forces_device) against tests/forces_ref.py of what load_buffers returns at that moment, every
output word (floats as words, one word per NaN): the batch's force scenes and the permuted five on one Engine each and against
BatchEngine.forces(); beams after cuts, breaks, delete passes, re-uploads and imports on every path and layout; a settled pile;
capacity above the scene; every combination of outputs; the host copy; reading changes nothing; the anchor -- forces() then one
substep: v == (push + beam) * dt, stress == tension / 20; the errors."""
import ctypes

import numpy as np
import pytest

import batch_forces_cases as bfc
import contacts_cases as cc
import forces_cases as fc
import forces_ref as fr
import report_harness as rh
from test_gpu_parity import ATOMIC, GRID, OFF, TILED, ALLPAIRS
from test_gpu_reupload import breaking_lattice, moved, without
from test_gpu_summary import READ_ONLY

pytestmark = pytest.mark.gpu
F = np.float32
ALL = dict(rows=True, beam_i32=True, tension=True, counts=True)


def make(sb, buf, bounds=1000.0, radius=10.0, subticks=64, **kw):
    """(engine with the scene uploaded, the scene as uploaded)"""
    kw.setdefault("collision_mode", OFF)
    up = cc.for_engine(sb, buf)
    return rh.engine(sb, up, bounds, particle_radius=radius, subticks=subticks, **kw), up


def call(eng, labels=None, other_body=False):
    import torch
    lab = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels)).to("cuda")
    f = eng.forces(labels=lab, other_body=other_body, **ALL)
    assert f.rows.dtype == torch.float32 and f.beam_i32.dtype == torch.int32 and f.counts.dtype == torch.int64
    return tuple(x.cpu().numpy() for x in f)   # (torch's stream waits: no sync)


def check(eng, upload, what, radius=10.0, subticks=64, labels=None, other_body=False):
    """forces() == forces_ref(load_buffers now); returns (the read-back, the expectation, what the engine gave)"""
    now = eng.load_buffers(upload.copy())
    exp = fr.forces_ref(now, radius, subticks, labels, other_body)
    got = call(eng, labels, other_body)
    fr.assert_forces(got, exp, what)
    return now, exp, got


# ---------------------------------------------------------------- the cases, and the batch twin
def test_every_scene_of_the_cases_and_the_batch_twin(sb):
    scenes = fc.engine_scenes(sb)
    twins = 0
    for name, buf, subticks in scenes:
        eng, up = make(sb, buf, subticks=subticks)
        _, exp, got = check(eng, up, name, subticks=subticks)
        lab = cc.striped_labels(up.max_particles)
        check(eng, up, name + ", labels given and not looked at", subticks=subticks, labels=lab)
        check(eng, up, name + ", other_body", subticks=subticks, labels=lab, other_body=True)
        again = call(eng)
        assert all(np.array_equal(fr.words(a), fr.words(b)) for a, b in zip(got, again)), name + ": two calls differ"
        eng.destroy()
        if up.max_particles <= 1024 and up.max_beams <= 4096:     # the batch twin: the same rows, beam_i32 and tension
            be = sb.BatchEngine(n_scenes=1, subticks=subticks, layout=up.layout, max_particles=up.max_particles, max_beams=up.max_beams)
            be.write_scene(up, 0, 1)
            bf = be.forces(**ALL)
            fr.assert_forces((bf.rows[0].cpu().numpy(), bf.beam_i32[0].cpu().numpy(), bf.tension[0].cpu().numpy(), None), got, name + ", the batch twin")
            assert bf.counts[0].cpu().numpy().tolist() == [int(x) for x in got[3]]
            be.destroy()
            twins += 1
    assert twins >= 30


def test_permuted_five_takes_the_partners_in_slot_order(sb):
    buf = fc.permuted_five(sb)
    for kw in (dict(collision_mode=OFF), dict(collision_mode=GRID, path=TILED), dict(collision_mode=ALLPAIRS, path=ATOMIC)):
        eng, up = make(sb, buf, **kw)
        _, exp, got = check(eng, up, "permuted five %s" % kw)
        wrong = fr.forces_ref(up, by_data_index=True)
        centre = int(up.mapping[0])
        assert (fr.words(got[0][centre, 2:6]) != fr.words(wrong[0][centre, 2:6])).any()
        eng.destroy()


@pytest.mark.parametrize("n", [0, 1])
def test_no_particle_and_one(sb, n):
    buf = bfc.scene(sb, (8, 4), np.asarray([(500.0, 500.0, 1.0, 2.0)], "f4")[:n], data_index=np.asarray([5][:n], np.int64))
    eng, up = make(sb, buf)
    _, exp, got = check(eng, up, "P = %d" % n)
    assert got[3].tolist() == [n, 0, 0, 0] and not fr.words(got[0]).any() and not got[1].any() and not fr.words(got[2]).any()
    eng.destroy()


@pytest.mark.parametrize("friction", [0.0, 0.7])
def test_friction_on_and_off_and_set_physics_constants(sb, friction):
    buf = bfc.contact_zoo(sb, 2, consts=dict(friction=friction, elasticity=0.9))
    eng, up = make(sb, buf)
    check(eng, up, "friction %g from the upload" % friction)
    eng.destroy()


# ---------------------------------------------------------------- beam counts, the gate, material modes
@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_beam_counts_round_a_wave_and_a_workgroup(sb, n):
    for gate in (False, True):
        buf = fc.beam_chain(sb, n, gate=gate)
        eng, up = make(sb, buf)      # (the far endpoints lie outside the bounds: clamped into the edge cells)
        _, exp, got = check(eng, up, "%d beams, gate %s" % (n, gate))
        assert got[3][1] == n
        eng.destroy()


@pytest.mark.parametrize("vary,expect_mode", [("none", 2), ("length", 1), ("spring", 0)])
def test_material_modes(sb, vary, expect_mode):
    """test_gpu_parity.py's three encodings of the tiled kernel's material dictionary: {spring, damp} come from the scene tables'
    own plane whichever the engine keeps"""
    buf = sb.scenes.lattice_buffers(48, 48, d=25.0, origin=(100.0, 100.0), jitter=2.0, layout=2, strain_limit=0.5)   # (6721 beams: more springs than the dictionary has rows)
    B = buf.beam_count
    rng = np.random.default_rng(17)
    if vary == "length":
        L = (buf.beams["length"][:B] * rng.uniform(0.97, 1.03, B)).astype("f4")
        buf.beams["length"][:B] = L
        buf.beams["target_length"][:B] = L
        buf.beams["last_length"][:B] = L
    if vary == "spring":
        buf.beams["spring"][:B] = rng.uniform(20, 60, B).astype("f4")
        buf.beams["damp"][:B] = rng.uniform(500, 800, B).astype("f4")
    eng, up = make(sb, buf, bounds=4000.0, path=TILED, tile_particles=256)
    assert eng.info("material_mode") == expect_mode
    _, exp, got = check(eng, up, "materials vary=%s" % vary)
    assert (got[2] != 0).sum() > B // 2
    eng.step(3)
    check(eng, up, "materials vary=%s, stepped" % vary)
    eng.destroy()


# ---------------------------------------------------------------- every path and layout, through breaks, cuts, uploads, imports
SCHEDULES = [("atomic", OFF, ATOMIC, {}), ("atomic, all pairs", ALLPAIRS, ATOMIC, {}), ("atomic, grid", GRID, ATOMIC, {}),
             ("tiled, one substep per launch", OFF, TILED, {"block_substeps": 1}), ("blocked", OFF, TILED, {}),
             ("tiled, grid", GRID, TILED, {"tile_particles": 256})]
CASES = [pytest.param(lay, *s, id="%s-v%d" % (s[0], lay)) for s in SCHEDULES for lay in (1, 2)]


@pytest.mark.parametrize("layout,what,mode,path,kw", CASES)
def test_every_path_and_layout_through_a_program(sb, layout, what, mode, path, kw):
    """a lattice thrown into the corner: yields, breaks, delete passes; a cut before and after the frame that deletes its beams; an odd
    and an even number of substeps; imports; a checkpoint and its restore; a plan-keeping upload that removed beams"""
    first = breaking_lattice(sb, layout=layout)
    eng, up = make(sb, first, bounds=4000.0, collision_mode=mode, path=path, **kw)
    check(eng, up, what + ", uploaded")
    eng.step(1)
    check(eng, up, what + ", 1 substep")
    eng.step(2)
    check(eng, up, what + ", 3 substeps")
    eng.checkpoint()
    eng.frame()
    now, exp, _ = check(eng, up, what + ", a frame")
    eng.cut(sb.engine.cut_shapes(segments=[(200.0, 0.0, 200.0, 4000.0)]))
    _, cut_exp, _ = check(eng, up, what + ", cut, flags pending")          # a pending flag still counts
    assert cut_exp[3][1] == exp[3][1]
    eng.frame()
    eng.frame()
    now, after, _ = check(eng, up, what + ", frames after the cut")
    assert after[3][1] < exp[3][1] and now.beam_count < first.beam_count   # the delete passes removed beams
    eng.step(5)
    check(eng, up, what + ", mid-frame")
    t = eng.state_tensors()
    t["beams"][:, 0] *= 1.001
    t["beams"][:, 1] *= 0.999
    eng.write_beams_device(t["beams"], target_length=True, last_length=True)
    t["particles"][:, 0:2] += 0.25
    eng.write_particles_device(t["particles"])
    check(eng, up, what + ", after the imports")
    eng.restore()
    check(eng, up, what + ", restored")
    del t
    cut = without(moved(first, 8), np.random.default_rng(11).random(first.beam_count) >= 0.01)
    eng.write_buffers(cut)
    check(eng, cut, what + ", an upload that removed beams")
    eng.frame()
    check(eng, cut, what + ", and a frame")
    eng.destroy()


@pytest.mark.parametrize("layout", [1, 2])
def test_plan_keeping_uploads(sb, layout):
    """test_gpu_state_io.py's sequence: an upload of the same topology and one that only removed beams both keep the plan; the
    caller's slots are then a subset of the engine's"""
    first = breaking_lattice(sb, layout=layout)
    eng, up = make(sb, first, bounds=4000.0, collision_mode=GRID)
    eng.frame()
    check(eng, up, "first")
    second = moved(first, 7)
    eng.write_buffers(second)
    assert eng.info("uploads_kept") == 1
    check(eng, second, "kept plan, before a step")
    eng.frame()
    check(eng, second, "kept plan")
    cut = without(moved(first, 8), np.random.default_rng(11).random(first.beam_count) >= 0.01)
    eng.write_buffers(cut)
    assert eng.info("uploads_edited") >= 1
    _, exp, _ = check(eng, cut, "removed beams, before a step")
    assert exp[3][1] == cut.beam_count < first.beam_count
    eng.frame()
    check(eng, cut, "removed beams, a frame")
    eng.step(5)
    check(eng, cut, "removed beams, mid-frame")
    eng.destroy()


def test_hybrid_quiet_lattice(sb):
    buf = sb.scenes.lattice_buffers(48, 40, d=30.0, origin=(300.0, 900.0), jitter=1.0, layout=2, velocity=(0.4, -1.0))
    eng, up = make(sb, buf, bounds=6000.0, collision_mode=GRID)
    for k in range(3):
        eng.frame()
        check(eng, up, "hybrid, frame %d" % k)
    eng.step(3)
    check(eng, up, "hybrid, mid-frame")
    eng.destroy()


def test_settled_pile_under_the_grid(sb):
    buf, bounds = sb.scenes.blob_pile_buffers(10, 8, gap=19.5)
    assert 2500 <= buf.particle_count <= 4000
    eng, up = make(sb, buf, bounds=bounds, collision_mode=GRID)
    for _ in range(3):
        eng.frame()
    bl = eng.bodies(counts=False)[0]
    _, exp, got = check(eng, up, "pile")
    assert exp[3][2] > 0 and np.abs(exp[0][:, 2:4]).max() > 0        # blobs still press on each other
    labels = bl.cpu().numpy()
    _, cross, _ = check(eng, up, "pile, other_body", labels=labels, other_body=True)
    assert 0 < cross[3][2] <= exp[3][2]          # (inside a blob the particles are 30 apart: what touches is another body's)
    f = eng.forces(labels=True, other_body=True, **ALL)                  # bodies() first, on the same stream
    fr.assert_forces(tuple(x.cpu().numpy() for x in f), cross, "pile, labels=True")
    eng.destroy()


# ---------------------------------------------------------------- degenerate geometry
def test_degenerate_geometry(sb):
    for n, ok in ((4096, True), (4097, False)):
        pts = np.zeros((n, 2), "f4")
        pts[:, 0] = 100.0 + 0.125 * (np.arange(n) // 2)       # two particles on every spot
        pts[:, 1] = 500.0
        buf, D = cc.free_scene(sb, n + 3, pts, seed=50)
        eng, up = make(sb, buf, radius=1.0e-20)
        if ok:
            assert eng.info("forces_cells_per_side") == 1
            _, exp, got = check(eng, up, "all pairs of %d" % n, radius=1.0e-20)
            assert got[3][2] == n and (got[0][D, 7] == 1.0).all()
        else:
            with pytest.raises(sb.EngineError) as e:
                eng.forces()
            assert e.value.status == 6      # SB_ERR_UNSUPPORTED
        eng.destroy()


# ---------------------------------------------------------------- capacity, outputs, the host copy, a side stream
def test_capacity_above_the_scene_and_every_combination_of_outputs(sb):
    import torch
    src = bfc.recap(sb, bfc.beam_kinds(sb), (300, 70))
    zoo = bfc.contact_zoo(sb, 2, cap=(300, 70))
    P0 = src.particle_count
    for s, d in enumerate(zoo.mapping[:zoo.particle_count].astype(int)):      # the zoo beside the beams: free data indices from 8 on
        src.particles[8 + s] = zoo.particles[d]
        src.mapping[P0 + s] = 8 + s
    src.particle_count = P0 + zoo.particle_count
    eng, up = make(sb, src)
    maxp, maxb = up.max_particles, up.max_beams
    _, exp, got = check(eng, up, "capacity 300 / 70")
    live = np.zeros(maxp, bool)
    live[up.mapping[:up.particle_count].astype(int)] = True
    assert not fr.words(got[0][~live]).any() and not got[1][~live].any() and not fr.words(got[2][3:]).any() and got[3][2] > 0
    sent = 0x7FBADBAD
    shapes = ((maxp, 8), (maxp, 2), (maxb,), (4,))
    for mask in range(1, 16):
        bufs = [torch.full((int(np.prod(sh)) + 3,), sent if k != 3 else -77, dtype=torch.int64 if k == 3 else torch.int32, device="cuda")
                if mask >> k & 1 else None for k, sh in enumerate(shapes)]
        views = [None if b is None else (b if k in (1, 3) else b.view(torch.float32)) for k, b in enumerate(bufs)]
        f = eng.forces(rows=views[0], beam_i32=views[1], tension=views[2], counts=views[3])
        outs = []
        for k, sh in enumerate(shapes):
            if bufs[k] is None:
                assert f[k] is None, mask
                outs.append(None)
                continue
            n = int(np.prod(sh))
            assert tuple(f[k].shape) == sh and f[k].data_ptr() == bufs[k].data_ptr(), mask
            assert (bufs[k][n:] == (-77 if k == 3 else sent)).all(), (mask, k)           # nothing behind the output
            outs.append(f[k].cpu().numpy())
        fr.assert_forces(tuple(outs), exp, "outputs %d" % mask)
    # rows at a pointer that is 4-byte and not 16-byte aligned
    mem = torch.full((maxp * 8 + 8,), sent, dtype=torch.int32, device="cuda")
    assert mem.data_ptr() % 16 == 0
    eng.forces(rows=mem.data_ptr() + 4)
    eng.sync()
    got_rows = mem[1:1 + maxp * 8].cpu().numpy().view("f4").reshape(maxp, 8)
    assert np.array_equal(fr.words(got_rows), fr.words(exp[0])) and int(mem[0]) == sent and (mem[1 + maxp * 8:] == sent).all()
    # the host copy; a side stream of a second engine's own
    lab = cc.striped_labels(maxp)
    host = eng.forces_host()
    assert host.rows.dtype == np.float32 and host.beam_i32.dtype == np.int32 and host.tension.dtype == np.float32 and host.counts.dtype == np.int64
    fr.assert_forces(tuple(host), exp, "host copy")
    cross = fr.forces_ref(up, labels=lab, other_body=True)
    fr.assert_forces(tuple(eng.forces_host(labels=lab, other_body=True)), cross, "host copy, other_body")
    other = sb.Engine(bounds_size=1000.0, layout=2, max_particles=4, max_beams=4, collision_mode=OFF)
    side = torch.cuda.ExternalStream(other.stream(), device=torch.device("cuda", eng.device))
    with torch.cuda.stream(side):
        f = eng.forces(**ALL)
        total = f.rows[:, 7].sum()
        kept = tuple(x.clone() for x in f)
    side.synchronize()
    fr.assert_forces(tuple(x.cpu().numpy() for x in kept), exp, "side stream")
    assert float(total) == float(exp[0][:, 7].sum()) > 0
    del side
    other.destroy()
    eng.destroy()


# ---------------------------------------------------------------- reading changes nothing
@pytest.mark.parametrize("what,mk,kw", READ_ONLY, ids=[r[0] for r in READ_ONLY])
def test_read_only(sb, what, mk, kw):
    def engine(sb, case, **kw):
        return rh.engine(sb, case["buf"], case["bounds"], **kw)

    def calls(eng, case):
        eng.forces(**ALL)
        eng.forces(labels=True, other_body=True, rows=True, counts=True)
        eng.forces_host()
    rh.read_only(sb, what, mk, kw, engine, calls, keys=("grid_builds", "grid_cells", "grid_wide"))


def test_read_only_on_a_contact_scene(sb):
    buf, bounds = sb.scenes.blob_pile_buffers(10, 8, gap=19.5)      # test_settled_pile_under_the_grid's: contacts after three frames
    case = dict(buf=buf, bounds=bounds)

    def engine(sb, case, **kw):
        eng = rh.engine(sb, case["buf"], case["bounds"], **kw)
        eng.frame()
        eng.frame()
        return eng

    def calls(eng, case):
        f = eng.forces(**ALL)
        assert int(f.counts[2]) > 0
        eng.forces_host()
    rh.read_only(sb, "pile", lambda sb: case, dict(collision_mode=GRID), engine, calls, keys=("grid_builds",))


# ---------------------------------------------------------------- the anchor
ANCHOR = [("beams only", OFF, ATOMIC, {}), ("beams only", OFF, TILED, {"block_substeps": 1}), ("beams only", OFF, TILED, {}),
          ("beams only", GRID, None, {}), ("contacts only", ALLPAIRS, ATOMIC, {}), ("contacts only", GRID, ATOMIC, {}),
          ("contacts only", GRID, TILED, {}), ("both", ALLPAIRS, ATOMIC, {}), ("both", GRID, ATOMIC, {}), ("both", GRID, TILED, {})]


@pytest.mark.parametrize("name,mode,path,kw", ANCHOR, ids=["%s mode %d path %s %s" % (n, m, p, "".join(k)) for n, m, p, k in ANCHOR])
def test_one_substep_applies_exactly_these_forces(sb, name, mode, path, kw):
    """gravity 0, drag 0, everything at rest: forces() then step(1) leaves v == (push + beam) * dt and stress == tension / 20"""
    buf = bfc.anchor_scenes(sb)[name]
    eng, up = make(sb, buf, collision_mode=mode, **(dict(kw) if path is None else dict(kw, path=path)))
    _, exp, got = check(eng, up, "anchor " + name)
    assert (got[3][1] > 0) == (name != "contacts only") and (got[3][2] > 0) == (name != "beams only")
    eng.step(1)
    after = eng.load_buffers(up.copy())
    idx = up.mapping[:up.particle_count].astype(int)
    assert np.isfinite(after.particles[idx]).all() and ((after.particles[idx, :2] > 10.0) & (after.particles[idx, :2] < 990.0)).all()
    want_v = (got[0][idx, 2:4] + got[0][idx, 0:2]) * F(2.0 ** -6)
    assert want_v.dtype == F and np.abs(want_v).max() > 0
    assert np.array_equal(fr.words(after.particles[idx, 2:4]), fr.words(want_v)), name
    bd = up.mapping[up.max_particles:up.max_particles + up.beam_count].astype(int)
    assert np.array_equal(fr.words(after.beams["stress"][bd]), fr.words(got[2][bd] * (F(1.0) / F(20.0)))), name
    eng.destroy()


# ---------------------------------------------------------------- errors, info
def test_errors_with_nothing_enqueued(sb):
    import torch
    buf = bfc.contact_zoo(sb)
    up = cc.for_engine(sb, buf)
    eng = sb.Engine(bounds_size=1000.0, layout=up.layout, max_particles=up.max_particles, max_beams=up.max_beams, collision_mode=OFF)
    for f in (eng.forces, eng.forces_host):
        with pytest.raises(sb.EngineError) as e:
            f()
        assert e.value.status == 5          # SB_ERR_STATE
    eng.write_buffers(up)
    mem = torch.full((8 * up.max_particles + 64,), -77, dtype=torch.int32, device="cuda")
    bad = (dict(rows=False), dict(other_body=True), dict(rows=mem.data_ptr() + 2), dict(labels=mem.data_ptr() + 1), dict(rows=False, counts=mem.data_ptr() + 4),
           dict(rows=False, beam_i32=mem.data_ptr() + 1), dict(rows=False, tension=mem.data_ptr() + 3))
    for kw in bad:
        with pytest.raises(sb.EngineError) as e:
            eng.forces(**kw)
        assert e.value.status == 1, kw      # SB_ERR_INVALID
    L, vp = sb.engine.load_library(), ctypes.c_void_p
    o = sb.engine.SbForcesOptions()
    size = ctypes.sizeof(o)
    for ssize, flags, reserved in ((size - 4, 0, 0), (size + 8, 0, 0), (size, 2, 0), (size, 0, 7), (size, 1, 0)):
        o.struct_size, o.flags, o.reserved[5] = ssize, flags, reserved
        assert L.sb_forces_device(eng._h, ctypes.byref(o), None, vp(mem.data_ptr()), None, None, None) == 1, (ssize, flags, reserved)
        host = np.empty((up.max_particles, 8), np.float32)
        assert L.sb_forces(eng._h, ctypes.byref(o), None, host.ctypes.data_as(vp), None, None, None) == 1, (ssize, flags, reserved)
    assert L.sb_forces_device(eng._h, None, None, None, None, None, None) == 1
    eng.sync()
    assert (mem == -77).all()               # nothing was enqueued
    o.struct_size, o.flags, o.reserved[5] = 0, 2, 7          # struct_size 0: all defaults, nothing else is read
    assert L.sb_forces_device(eng._h, ctypes.byref(o), None, vp(mem.data_ptr()), None, None, None) == 0   # ... and the engine still works
    d = [int(x) for x in up.mapping[:4]]
    eng.halo_configure(d[:2], d[2:])
    with pytest.raises(sb.EngineError) as e:
        eng.forces()
    assert e.value.status == 6              # SB_ERR_UNSUPPORTED
    eng.destroy()


def test_info_keys(sb):
    s = cc.big_scene(sb, "64 cells per side")
    eng, up = make(sb, s["buf"], bounds=s["bounds"])
    assert eng.info("forces_kernel_scratch_bytes") == 0 and 0 < eng.info("forces_kernel_vgprs") <= 64
    assert eng.info("forces_table_build_us") == 0 and eng.info("forces_cells_per_side") == 64
    check(eng, up, "64 cells per side")
    built = eng.info("forces_table_build_us")
    assert built > 0
    eng.forces()
    assert eng.info("forces_table_build_us") == built       # no upload, no table build
    eng.write_buffers(up)                                   # an upload drops the tables
    check(eng, up, "after the second upload")
    eng.destroy()
