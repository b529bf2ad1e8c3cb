"""Engine.cut (sb_cut_device / sb_cut) on the GPU: `hit` and `counts` equal tests/cut_ref.py on the case table and
on scenes, on every path and on both halves of the double buffer; a cut is the flag the substep would have raised, so the run after
it equals the oracle's with the same bits set in its delete mask, bit for bit; and the reports, the checkpoint and the uploads
see a cut as they see a beam that broke."""
import ctypes

import numpy as np
import pytest

import cut_cases
import cut_ref
from test_gpu_parity import ATOMIC, GRID, OFF, TILED, assert_same

pytestmark = pytest.mark.gpu

PATHS = [
    ("blocked", OFF, TILED, {}),
    ("one substep per launch", OFF, TILED, {"block_substeps": 1, "tile_particles": 256}),
    ("atomic", OFF, ATOMIC, {}),
    ("default", GRID, 0, {}),
]
IDS = [p[0] for p in PATHS]
ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 5, 6


def engine(sb, buf, bounds, mode, path, kw):
    eng = sb.Engine(bounds_size=bounds, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=mode,
                    path=path, **kw)
    eng.write_buffers(buf)
    return eng


def dev_shapes(shapes):
    import torch
    return torch.from_numpy(np.ascontiguousarray(shapes).view(np.int32)).cuda()


def cut(eng, shapes, **kw):
    """(hit uint8 [max_beams] with 0 where nothing was written, counts list) of a cut with device shapes"""
    hit, counts = eng.cut(dev_shapes(shapes), hit=True, **kw)
    return hit.cpu().numpy(), counts.cpu().numpy().tolist()


def state(eng, buf):
    return eng.load_buffers(buf.copy())


def final(eng, buf):
    return state(eng, buf), eng.counts(), eng.info("substeps_done")


def same_run(a, b, what):
    assert_same(a[0], b[0], what)
    assert a[1:] == b[1:], (what, a[1:], b[1:])


def has_two_tiles(eng, buf, what):
    """the plan has at least two tiles and beams with copies (entries) in two of them"""
    assert eng.info("tiles") >= 2 and eng.info("beam_copies") > buf.beam_count, (what, eng.info("tiles"), eng.info("beam_copies"))


# ---------------------------------------------------------------- 1. predicate parity

@pytest.mark.parametrize("what,mode,path,kw", PATHS, ids=IDS)
def test_case_table(sb, what, mode, path, kw):
    """every shape of the table against every beam of the table (non-finite coordinates arrive through the particle import)"""
    import torch
    buf, records = cut_cases.table_scene(sb)
    eng = engine(sb, buf, 1000.0, mode, path, kw)
    eng.write_particles_device(torch.from_numpy(records).cuda())
    shapes, A, B = cut_cases.table_arrays()
    n = len(shapes)
    for k in range(n):
        hit, counts = cut(eng, shapes[k:k + 1], dry_run=True)
        want = cut_ref.hits(shapes[k:k + 1], A, B)
        assert np.array_equal(hit[:n] != 0, want), (cut_cases.TABLE[k][0], np.flatnonzero((hit[:n] != 0) != want))
        assert counts == [n, int(want.sum()), 0, 0] and not hit[n:].any(), cut_cases.TABLE[k][0]
        if cut_cases.TABLE[k][4] is not None:
            assert bool(hit[k]) == cut_cases.TABLE[k][4], cut_cases.TABLE[k][0]
    hit, counts = cut(eng, shapes, dry_run=True)   # all of them in one call
    assert np.array_equal(hit[:n] != 0, cut_ref.hits(shapes, A, B)) and counts[2:] == [0, 0]
    assert eng.info("beams_flagged") == 0 and eng.info("cuts") == n + 1
    eng.destroy()


@pytest.mark.parametrize("scene", list(cut_cases.SCENES))
@pytest.mark.parametrize("substeps", [0, 3])
@pytest.mark.parametrize("what,mode,path,kw", PATHS, ids=IDS)
def test_scene_parity(sb, what, mode, path, kw, scene, substeps):
    """hit and counts == cut_ref on the state read back at that point, after 0 and after an odd number of substeps (the other half
    of the double buffer); the first case cuts for real, the others are dry runs on the same engine; untouched indices stay"""
    import torch
    buf, bounds = cut_cases.SCENES[scene](sb)
    eng = engine(sb, buf, bounds, mode, path, kw)
    if scene == "lattice" and path == TILED:
        has_two_tiles(eng, buf, what)
    if substeps:
        eng.step(substeps)
    assert eng.info("beams_flagged") == 0, "nothing may have broken yet: the counts below assume it"
    now = state(eng, buf)
    cases = cut_cases.scene_shapes(cut_cases.box_of(now))
    for name, shapes in cases.items():
        want_hit, want = cut_ref.scene_ref(now, shapes, dry=True)
        hit = torch.full((buf.max_beams,), 0xA5, dtype=torch.uint8, device="cuda")
        _, counts = eng.cut(dev_shapes(shapes), dry_run=True, hit=hit)
        hit = hit.cpu().numpy()
        used = np.zeros(buf.max_beams, dtype=bool)
        used[buf.mapping[buf.max_particles:buf.max_particles + buf.beam_count].astype(np.int64)] = True
        assert np.array_equal(hit[used], want_hit[used]), (what, name)
        assert (hit[~used] == 0xA5).all() and (~used).any(), (what, name, "indices of no beam must not be written")
        assert counts.cpu().numpy().tolist() == want, (what, name)
    assert eng.info("beams_flagged") == 0
    name = "stroke, none, disc"
    want_hit, want = cut_ref.scene_ref(now, cases[name])
    hit, counts = cut(eng, cases[name])
    assert np.array_equal(hit, want_hit) and counts == want, (what, name, counts, want)
    flagged = eng.info("beams_flagged")   # (a bit per copy the layout keeps)
    assert flagged >= want[1], (what, flagged, want)
    if scene == "lattice" and "tile_particles" in kw:
        assert flagged > want[1], "a hit beam must have copies in two tiles: %d bits for %d beams" % (flagged, want[1])
    row, sums = eng.summary(counts=True)
    assert int(sums[3]) == want[1], "summary: pending flags"
    eng.destroy()


@pytest.mark.parametrize("what,mode,path,kw", PATHS[:2], ids=["blocked plan", "tiled plan"])
def test_strokes_along_every_lattice_line(sb, what, mode, path, kw):
    """The knife along the tile boundaries.  sb_get_info does not say where a plan's tiles meet, so the knife is laid along EVERY
    line between two neighbouring columns and between two neighbouring rows of the lattice, one stroke a call, for real: wherever
    the plan's tiles meet, the beams that cross from one tile into the other cross one of these lines (a horizontal beam a column
    line, a vertical one a row line, a diagonal both), so every beam with copies (tiled plan) or entries (blocked plan) in two
    tiles is hit by some stroke -- asserted: the strokes together hit every beam, and sb_get_info says that the plan has two
    tiles and more copies / entries than beams.  Per stroke: hit and counts equal the reference, the delete pass removes exactly
    the hit beams, and a restore goes back.  On the tiled plan a hit beam with two copies shows as two pending bits."""
    import torch
    buf, bounds = cut_cases.SCENES["lattice"](sb)
    eng = engine(sb, buf, bounds, mode, path, kw)
    has_two_tiles(eng, buf, what)
    x0, y0, x1, y1 = cut_cases.box_of(buf)
    lines = [(cut_ref.SEGMENT, 30.0 + 30.0 * (i + 0.5), y0 - 5, 30.0 + 30.0 * (i + 0.5), y1 + 5) for i in range(39)]
    lines += [(cut_ref.SEGMENT, x0 - 5, 30.0 + 30.0 * (j + 0.5), x1 + 5, 30.0 + 30.0 * (j + 0.5)) for j in range(29)]
    used = np.zeros(buf.max_beams, dtype=bool)
    used[buf.mapping[buf.max_particles:buf.max_particles + buf.beam_count].astype(np.int64)] = True
    eng.checkpoint()
    union, extra_bits = np.zeros(buf.max_beams, dtype=bool), []
    for line in lines:
        stroke = cut_ref.pack([line])
        want_hit, want = cut_ref.scene_ref(buf, stroke)
        hit, counts = cut(eng, stroke)
        assert np.array_equal(hit, want_hit) and counts == want and 0 < want[1] < want[0], (what, line, counts, want)
        extra_bits.append(eng.info("beams_flagged") - want[1])
        eng.delete_pass()
        assert eng.counts()[1] == buf.beam_count - want[1], (what, line)
        alive = torch.zeros(buf.max_beams, dtype=torch.uint8, device="cuda")
        eng.read_state_device(beam_alive=alive)
        assert np.array_equal(alive.cpu().numpy()[used] == 0, want_hit[used] == 1), (what, line)
        union |= want_hit == 1
        eng.restore()
        assert eng.counts()[1] == buf.beam_count and eng.info("beams_flagged") == 0
    assert np.array_equal(union, used), "every beam crosses a line: the two-tile beams are among the beams hit"
    print("%s: pending bits beyond one per hit beam, per stroke: %s" % (what, extra_bits))
    if "tile_particles" in kw:
        assert max(extra_bits) > 0 and min(extra_bits) >= 0, "hit beams with copies in two tiles show as two bits"
    else:
        assert set(extra_bits) == {0}, "the blocked layout keeps one bit per beam, whatever its entries"
    eng.destroy()


@pytest.mark.parametrize("what,mode,path,kw", PATHS, ids=IDS)
def test_dry_run_changes_nothing(sb, what, mode, path, kw):
    buf, bounds = cut_cases.SCENES["lattice"](sb)
    out = {}
    for k in ("plain", "dry"):
        eng = engine(sb, buf, bounds, mode, path, kw)
        eng.frame()
        eng.step(5)
        if k == "dry":
            for shapes in cut_cases.scene_shapes(cut_cases.box_of(state(eng, buf))).values():
                eng.cut(dev_shapes(shapes), dry_run=True, hit=True)
        out[k] = [eng.info("beams_flagged"), final(eng, buf)]
        eng.step(eng.subticks - 5)
        eng.delete_pass()
        eng.frame()
        out[k].append(final(eng, buf))
        eng.destroy()
    assert out["plain"][0] == out["dry"][0]
    same_run(out["dry"][1], out["plain"][1], what + ": right after the dry runs")
    same_run(out["dry"][2], out["plain"][2], what + ": the following frames")


# ---------------------------------------------------------------- 2. oracle parity

def flag_in_oracle(ref, buf, shapes):
    """set the bits of the reference's delete mask for every live slot the reference predicate hits, on the oracle's own state"""
    now = ref.load_buffers(buf.copy())
    _, A, B = cut_ref.beam_ends(now)
    slots = np.flatnonzero(cut_ref.hits(shapes, A, B))
    for s in slots:
        bit = buf.max_particles + int(s)
        ref.delete[bit >> 5] |= np.uint32(1 << (bit & 31))
    return len(slots)


def quiet_lattice(sb):
    return sb.scenes.lattice_buffers(128, 96, d=30.0, origin=(300.0, 900.0), jitter=1.0, layout=2, velocity=(0.4, -1.0)), 6000.0


def touching(sb):
    """two small blobs, one dropped onto the other: contacts from the first frames on"""
    parts, beams, base = [], [], 0
    for ox, oy, w, h in ((100.0, 12.0, 12, 6), (160.0, 200.0, 8, 5)):
        p, b = sb.scenes.rectangle(ox, oy, 24.0, w, h, 50.0, 400.0, 0.2, 0.8, base=base, layout=2)
        pv = np.zeros((len(p), 6), dtype=np.float32)
        pv[:, :2] = p
        pv[:, 3] = -60.0 if base else 0.0
        parts.append(pv)
        beams.append(b)
        base += len(p)
    buf = sb.Buffers(2, base + 4, sum(len(b) for b in beams) + 4)
    buf.set_scene(np.concatenate(parts), np.concatenate(beams))
    return buf, 1000.0


ORACLE_CASES = [pytest.param(*p, "lattice", id=p[0]) for p in PATHS] + [
    pytest.param("default", GRID, 0, {}, "quiet", id="hybrid, quiet"),
    pytest.param("default", GRID, 0, {}, "touching", id="default, touching"),
]


@pytest.mark.parametrize("substeps", [0, 7])
@pytest.mark.parametrize("what,mode,path,kw,scene", ORACLE_CASES)
def test_oracle_parity(sb, oracle, what, mode, path, kw, scene, substeps):
    """s substeps, the cut, the rest of the frame, one more frame == the oracle with the hit slots' delete bits set"""
    buf, bounds = {"lattice": cut_cases.SCENES["lattice"], "quiet": quiet_lattice, "touching": touching}[scene](sb)
    eng = engine(sb, buf, bounds, mode, path, kw)
    ref = oracle.OracleEngine(bounds, 10.0, 64, buf.layout, mode, threads=16)
    ref.write_buffers(buf)
    if scene == "quiet":   # (the hybrid needs a look at the scene before it runs blocked launches: a frame first)
        eng.frame()
        ref.frame()
    if substeps:
        eng.step(substeps)
        ref.step(substeps)
    shapes =cut_cases.scene_shapes(cut_cases.box_of(state(eng, buf)))["stroke, none, disc"]
    n = flag_in_oracle(ref, buf, shapes)
    _, counts = eng.cut(dev_shapes(shapes))
    counts = counts.cpu().numpy().tolist()
    assert counts[1] == n > 0 and counts[2] + counts[3] == n, (what, counts, n)
    eng.step(eng.subticks - substeps)
    ref.step(ref.subticks - substeps)
    eng.delete_pass()
    ref.delete_pass()
    assert_same(state(eng, buf), ref.load_buffers(buf.copy()), what + ": the frame of the cut")
    assert eng.counts()[1] <= buf.beam_count - n
    eng.frame()
    ref.frame()
    assert_same(state(eng, buf), ref.load_buffers(buf.copy()), what + ": one frame later")
    if scene == "quiet":
        assert eng.info("hybrid_launches") > 0
    eng.destroy()


@pytest.mark.parametrize("what,mode,path,kw", PATHS, ids=IDS)
def test_cut_then_delete_pass_alone(sb, oracle, what, mode, path, kw):
    """a cut at a frame boundary, then sb_delete_pass alone"""
    buf, bounds = cut_cases.SCENES["default"](sb)
    eng = engine(sb, buf, bounds, mode, path, kw)
    ref = oracle.OracleEngine(bounds, 10.0, 64, buf.layout, mode, threads=4)
    ref.write_buffers(buf)
    eng.frame()
    ref.frame()
    shapes = cut_cases.scene_shapes(cut_cases.box_of(state(eng, buf)))["horizontal stroke"]
    n = flag_in_oracle(ref, buf, shapes)
    hit, counts = cut(eng, shapes)
    assert counts == [buf.beam_count, n, n, 0] and n > 0
    eng.delete_pass()
    ref.delete_pass()
    assert_same(state(eng, buf), ref.load_buffers(buf.copy()), what + ": after the delete pass")
    assert eng.counts()[1] == buf.beam_count - n
    eng.frame()
    ref.frame()
    assert_same(state(eng, buf), ref.load_buffers(buf.copy()), what + ": one frame later")
    eng.destroy()


# ---------------------------------------------------------------- 3. interplay

def sheet(sb):
    """a 12 x 8 lattice at rest; x = 265 lies between its columns 5 (x = 250) and 6 (x = 280)"""
    return sb.scenes.lattice_buffers(12, 8, d=30.0, origin=(100.0, 100.0), layout=2, slack=5), 1000.0


@pytest.mark.parametrize("what,mode,path,kw", [PATHS[0], PATHS[3]], ids=["blocked", "default"])
def test_reports_see_a_cut_as_a_break(sb, what, mode, path, kw):
    import torch
    buf, bounds = sheet(sb)
    eng = engine(sb, buf, bounds, mode, path, kw)
    stroke = cut_ref.pack([(cut_ref.SEGMENT, 265.0, 0.0, 265.0, 900.0)])
    want_hit, want = cut_ref.scene_ref(buf, stroke)
    hit, counts = cut(eng, stroke)
    assert np.array_equal(hit, want_hit) and counts == want and want[1] > 0
    labels, bodies = eng.bodies()
    assert int(bodies[0]) == 1, "a pending flag still connects"
    assert int(eng.summary(counts=True)[1][3]) == want[1] and eng.info("beams_flagged") >= want[1]
    again = cut(eng, stroke)[1]                      # the same stroke twice
    assert again == [want[0], want[1], 0, want[1]], again
    eng.delete_pass()
    assert int(eng.bodies()[1][0]) == 2 and eng.info("beams_flagged") == 0
    alive = torch.full((buf.max_beams,), 7, dtype=torch.uint8, device="cuda")
    eng.read_state_device(beam_alive=alive)
    alive = alive.cpu().numpy()
    used = np.zeros(buf.max_beams, dtype=bool)
    used[buf.mapping[buf.max_particles:buf.max_particles + buf.beam_count].astype(np.int64)] = True
    assert np.array_equal(alive[used] == 0, want_hit[used] == 1)
    third = cut(eng, stroke)[1]                      # removed beams are not tested
    assert third == [want[0] - want[1], 0, 0, 0], third
    assert eng.info("cuts") == 3 and eng.info("cut_table_build_us") > 0 and 0 < eng.info("cut_kernel_vgprs") <= 512
    eng.destroy()


@pytest.mark.parametrize("what,mode,path,kw", PATHS, ids=IDS)
def test_checkpoint_cut_frame_restore(sb, what, mode, path, kw):
    """checkpoint -> cut -> frame -> restore -> frame == the run without the cut; a cut before the checkpoint is part of it"""
    buf, bounds = cut_cases.SCENES["lattice"](sb)
    N, C = (engine(sb, buf, bounds, mode, path, kw) for _ in range(2))
    for e in (N, C):
        e.frame()
        e.step(5)
    shapes = cut_cases.scene_shapes(cut_cases.box_of(state(C, buf)))
    C.checkpoint()
    _, counts = C.cut(dev_shapes(shapes["disc"]))
    assert int(counts[1]) > 0
    C.step(C.subticks - 5)
    C.delete_pass()
    cut_counts = C.counts()
    C.restore()
    for e in (N, C):
        e.step(e.subticks - 5)
        e.delete_pass()
    assert C.counts()[1] > cut_counts[1], "the cut must have removed beams the plain run keeps"
    same_run(final(C, buf), final(N, buf), what + ": restore undoes the cut")
    for e in (N, C):   # ... and a pending cut travels with a checkpoint
        e.step(3)
        e.cut(dev_shapes(shapes["vertical stroke"]))
    C.checkpoint()
    C.frame()
    C.restore()
    for e in (N, C):
        e.step(e.subticks - 3)
        e.delete_pass()
        e.frame()
    out = final(C, buf), final(N, buf)
    N.destroy()
    C.destroy()
    same_run(out[0], out[1], what + ": a pending cut in a checkpoint")


@pytest.mark.parametrize("what,mode,path,kw", [PATHS[0], PATHS[2], PATHS[3]], ids=["blocked", "atomic", "default"])
def test_after_an_upload_that_removed_beams(sb, oracle, what, mode, path, kw):
    """hit lands on the NEW data indices; beams the upload removed are not tested; the run equals the oracle's"""
    from test_gpu_reupload import moved, without
    first, bounds = cut_cases.SCENES["lattice"](sb)
    second = without(moved(first, 8), np.random.default_rng(11).random(first.beam_count) >= 0.02, shuffle_mapping=3)
    eng = engine(sb, first, bounds, mode, path, kw)
    eng.frame()
    eng.cut(dev_shapes(cut_cases.scene_shapes(cut_cases.box_of(first))["disc"]), dry_run=True)   # (tables of the first upload)
    eng.write_buffers(second)
    assert eng.info("uploads_edited") == 1 and second.beam_count < first.beam_count
    ref = oracle.OracleEngine(bounds, 10.0, 64, 2, mode, threads=16)
    ref.write_buffers(second)
    for e in (eng, ref):
        e.step(3)
    shapes = cut_cases.scene_shapes(cut_cases.box_of(state(eng, second)))["stroke, none, disc"]
    want_hit, want = cut_ref.scene_ref(state(eng, second), shapes)
    n = flag_in_oracle(ref, second, shapes)
    hit, counts = cut(eng, shapes)
    assert counts[0] == second.beam_count and counts[:2] == want[:2] and n == want[1] > 0, (counts, want)
    assert np.array_equal(hit, want_hit)
    for e in (eng, ref):
        e.step(e.subticks - 3)
        e.delete_pass()
        e.frame()
    assert_same(state(eng, second), ref.load_buffers(second.copy()), what)
    eng.destroy()


def status_of(call):
    from softbody_webgpu_amd.engine import EngineError
    with pytest.raises(EngineError) as ex:
        call()
    return ex.value.status


def test_errors(sb):
    import torch
    lib = sb.engine.load_library()
    vp = ctypes.c_void_p
    buf, bounds = cut_cases.SCENES["default"](sb)
    shapes = dev_shapes(cut_ref.pack([(1, 0, 0, 1000, 1000)] * 65))
    eng = sb.Engine(bounds_size=bounds, layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=OFF)
    assert status_of(lambda: eng.cut(shapes[:1])) == ERR_STATE                       # before an upload
    assert status_of(lambda: eng.cut([(1, 0, 0, 1000, 1000)])) == ERR_STATE
    assert status_of(lambda: eng.cut(shapes)) == ERR_INVALID                         # ... but the arguments come first
    eng.write_buffers(buf)
    o = sb.engine.SbCutOptions()
    counts = torch.zeros(5, dtype=torch.int64, device="cuda")
    ok = (32, 0, 0)
    for size, flags, reserved in ((31, 0, 0), (32, 2, 0), (32, 0, 1)):
        o.struct_size, o.flags, o.reserved[5] = size, flags, reserved
        assert lib.sb_cut_device(eng._h, ctypes.byref(o), vp(shapes.data_ptr()), 1, None, None) == ERR_INVALID
    o.struct_size, o.flags, o.reserved[5] = ok
    for ptr, n, cptr in ((shapes.data_ptr(), 65, None), (None, 1, None), (shapes.data_ptr() + 2, 1, None), (shapes.data_ptr(), 1, counts.data_ptr() + 4)):
        assert lib.sb_cut_device(eng._h, ctypes.byref(o), vp(ptr), n, None, vp(cptr)) == ERR_INVALID
    assert eng.info("beams_flagged") == 0 and eng.info("cuts") == 0
    for bad in ([(3, 0, 0, 1, 1)], [(2, 0, 0, 5, 1)]):                                # sb_cut sees the shapes
        rows = cut_ref.pack(bad)
        assert lib.sb_cut(eng._h, None, rows.ctypes.data_as(vp), 1, None, None) == ERR_INVALID
        hit, c = eng.cut(dev_shapes(rows), hit=True)                                  # ... sb_cut_device ignores them
        assert c.cpu().numpy().tolist() == [buf.beam_count, 0, 0, 0] and not hit.any()
    with pytest.raises(ValueError):
        eng.cut(torch.zeros((1, 8), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        eng.cut(torch.zeros((1, 8), dtype=torch.int32))
    eng.destroy()
    small = sb.scenes.default_buffers(2, 256, 512)
    eng = sb.Engine(layout=2, max_particles=256, max_beams=512, collision_mode=OFF, path=TILED)
    eng.write_buffers(small)
    eng.halo_configure([0, 1], [2, 3])
    assert status_of(lambda: eng.cut(shapes[:1])) == ERR_UNSUPPORTED                 # ghost zones
    eng.destroy()


# ---------------------------------------------------------------- 4. shape counts; the host variant

@pytest.mark.parametrize("what,mode,path,kw", [PATHS[0], PATHS[3]], ids=["blocked", "default"])
def test_shape_counts_and_the_host_variant(sb, what, mode, path, kw):
    buf, bounds = cut_cases.SCENES["lattice"](sb)
    D, H = (engine(sb, buf, bounds, mode, path, kw) for _ in range(2))
    for e in (D, H):
        e.step(3)
    now = state(D, buf)
    cases = cut_cases.scene_shapes(cut_cases.box_of(now))
    none = np.zeros((0, 8), dtype=np.uint32)
    for shapes in (none, cases["vertical stroke"], cases["64 shapes"]):               # 0, 1 and 64 shapes
        want_hit, want = cut_ref.scene_ref(now, shapes, dry=True)
        dh, dc = cut(D, shapes, dry_run=True)
        hh, hc = H.cut(shapes, dry_run=True, hit=True)
        assert np.array_equal(dh, want_hit) and dc == want and want[0] == buf.beam_count, (what, len(shapes))
        assert np.array_equal(hh, dh) and hc.tolist() == dc, (what, len(shapes))
    float_rows = np.zeros((64, 8), dtype=np.float32)                                  # a float32 tensor: the kind as a number
    float_rows[:, 0] = cases["64 shapes"][:, 0]
    float_rows[:, 1:5] = cases["64 shapes"][:, 1:5].view(np.float32)
    import torch
    fh, fc = D.cut(torch.from_numpy(float_rows).cuda(), dry_run=True, hit=True)
    assert np.array_equal(fh.cpu().numpy(), cut_ref.scene_ref(now, cases["64 shapes"])[0])
    # for real: the list form goes through sb_cut; both engines then run the same
    rows = [(int(k), *np.asarray(xy).view(np.float32).tolist()) for k, xy in zip(cases["64 shapes"][:, 0], cases["64 shapes"][:, 1:5])]
    hh, hc = H.cut(rows, hit=True)
    dh, dc = cut(D, cases["64 shapes"])
    assert np.array_equal(hh, dh) and hc.tolist() == dc and dc[2] == dc[1] > 0
    for e in (D, H):
        e.step(e.subticks - 3)
        e.delete_pass()
        e.frame()
    out = final(D, buf), final(H, buf)
    D.destroy()
    H.destroy()
    same_run(out[0], out[1], what + ": sb_cut and sb_cut_device")
    assert out[0][1][1] <= buf.beam_count - dc[1]


# ---------------------------------------------------------------- 5. the Node host

from test_node_host import needs_node, run_node  # noqa: E402


@needs_node
def test_node_cut_equals_pythons(sb):
    """host/test/cut.gpu.test.js checks engine.cut against its own Math.fround restatement and the bodies afterwards; its counts and
    hit bytes are also those of cut_ref and of Engine.cut on the same scene, capacity and shapes"""
    r = run_node("cut.gpu.test.js")
    assert r["ok"], r
    buf = sb.scenes.default_buffers(2, 128, 320)
    shapes = sb.cut_shapes(segments=[(685, 0, 685, 100)], discs=[(150, 165, 40)])
    want_hit, want = cut_ref.scene_ref(buf, shapes)
    assert r["counts"] == want and r["hit"] == want_hit.tolist()
    eng = sb.Engine(bounds_size=1000.0, layout=2, max_particles=128, max_beams=320, collision_mode=OFF)
    eng.write_buffers(buf)
    hit, counts = cut(eng, shapes)
    assert counts == r["counts"] and hit.tolist() == r["hit"]
    eng.frame()
    assert int(eng.bodies()[1][0]) == r["bodiesAfter"] > r["bodiesBefore"]
    eng.destroy()
