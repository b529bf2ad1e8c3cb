"""Engine.contacts() (sb_contacts_device) against tests/contacts_ref.py, exactly: every scene of the batch's contact
cases on one Engine each (and against BatchEngine.contacts() where it fits), scenes beyond one workgroup and one scan block, the
pair list and its truncation, a settling pile on every path against an oracle that ran the same program, reading changes
nothing, positions at the call's place in the stream, every combination of outputs, the degenerate scenes and the errors."""
import ctypes
import json

import numpy as np
import pytest

import batch_harness as bh
import contacts_cases as cc
import contacts_ref as cref
import report_harness as rh
import summary_cases as sc
from test_gpu_parity import ATOMIC, GRID, OFF, TILED, ALLPAIRS, assert_same
from test_gpu_summary import READ_ONLY
from test_node_host import needs_node, run_node

pytestmark = pytest.mark.gpu


def engine(sb, scene, **kw):
    kw.setdefault("collision_mode", OFF)
    return rh.engine(sb, cc.for_engine(sb, scene["buf"]), scene["bounds"], particle_radius=scene.get("radius", 10.0), **kw)


def brief(counts):
    return tuple(int(x) for x in counts)


def assert_contacts(got, exp, what):
    """(touch, pairs or None, counts) by value"""
    touch, pairs, counts = got
    print(what, "counts", brief(counts), "expected", brief(exp[2]))
    assert brief(counts) == brief(exp[2]), "%s: counts %s, expected %s" % (what, brief(counts), brief(exp[2]))
    bad = np.flatnonzero((np.asarray(touch) != exp[0]).any(axis=1))
    assert bad.size == 0, "%s: %d touch rows differ, first %d: %s, expected %s" % (what, bad.size, bad[0], touch[bad[0]], exp[0][bad[0]])
    if pairs is not None:
        bad = np.flatnonzero((np.asarray(pairs) != exp[1]).any(axis=1))
        assert bad.size == 0, "%s: %d pairs differ, first row %d: %s, expected %s" % (what, bad.size, bad[0], pairs[bad[0]], exp[1][bad[0]])


def call(eng, labels=None, pairs=0, other_body=False):
    import torch
    lab = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels)).to("cuda")
    out = eng.contacts(labels=lab, pairs=pairs, other_body=other_body)
    assert out[1].dtype == torch.int64 and out[0].dtype == torch.int32
    return out[0].cpu().numpy(), (out[2].cpu().numpy() if pairs else None), out[1].cpu().numpy()   # (torch's stream waits: no sync)


# 1
def test_every_scene_of_the_batch_cases_on_one_engine(sb, oracle):
    import torch
    scenes = cc.batch_scenes(sb)
    assert len(scenes) >= 30
    checked_batch = 0
    for s in scenes:
        buf = s["buf"]
        now = buf
        if s["finite"]:      # what an oracle's load_buffers returns after the same (empty) program
            ref = oracle.OracleEngine(s["bounds"], s["radius"], 64, buf.layout, 0, threads=1)
            ref.write_buffers(buf)
            now = ref.load_buffers(buf.copy())
        lab = cc.striped_labels(buf.max_particles)
        eng = engine(sb, s)
        for labels, m, other in ((None, 0, False), (lab, 12000 if s["radius"] == 600.0 else 40, False), (lab, 40, True)):
            exp = cref.contacts_ref(now, s["radius"], s["bounds"], labels, m, other)
            assert_contacts(call(eng, labels, m, other), exp, "%s, %d pairs, other_body %s" % (s["name"], m, other))
        if s["radius"] == 600.0:
            assert eng.info("contacts_cells_per_side") == 1 and exp[2][0] == 10296
        eng.destroy()
        if s["fits_batch"]:
            be = sb.BatchEngine(n_scenes=1, bounds_size=s["bounds"], particle_radius=s["radius"], layout=buf.layout, max_particles=buf.max_particles,
                                max_beams=buf.max_beams)
            be.write_scene(buf, 0, 1)
            bt, bcnt, bp = be.contacts(labels=torch.from_numpy(lab[None, :].copy()).to("cuda"), pairs=40)
            exp = cref.contacts_ref(now, s["radius"], s["bounds"], lab, 40)
            assert_contacts((bt.cpu().numpy()[0], bp.cpu().numpy()[0], bcnt.cpu().numpy()[0].astype(np.int64)), exp, s["name"] + ", the batch")
            be.destroy()
            checked_batch += 1
    assert checked_batch >= 20


# 2
@pytest.mark.parametrize("path", [None, ATOMIC], ids=["default", "atomic"])
@pytest.mark.parametrize("name", list(cc.BIG))
def test_beyond_one_workgroup_and_one_scan_block(sb, name, path):
    s = cc.big_scene(sb, name)
    maxp = s["buf"].max_particles
    lab = cc.striped_labels(maxp)
    eng = engine(sb, s, **({} if path is None else dict(path=path)))
    assert eng.info("contacts_cells_per_side") == cc.cells_per_side(s["bounds"], s["radius"], s["buf"].particle_count)
    n = 2000
    exp = cc.expected(s, lab, n, key="striped %d" % n)
    assert_contacts(call(eng, lab, n), exp, name)
    exp = cc.expected(s, None, 0, key="plain")
    assert_contacts(call(eng), exp, name + ", no labels")
    eng.destroy()


# 2b (tests/test_contacts_cpu.py: what the two scenes reach, and that a scan without its carry gives other words there)
@pytest.mark.parametrize("name", list(cc.PAST))
def test_past_256_scan_blocks(sb, name):
    """more than 256 blocks in the scan of the cell counts ("544 cells per side") and in the 64-bit scan over the data indices
    that places the pair list ("indices past 2^18"): the second trip of the loop over the block sums, with its carry"""
    s = cc.big_scene(sb, name)
    lab = cc.striped_labels(s["buf"].max_particles)
    eng = engine(sb, s)
    assert eng.info("contacts_cells_per_side") == cc.cells_per_side(s["bounds"], s["radius"], s["buf"].particle_count)
    exp = cc.expected(s, None, 0, key="plain")
    assert_contacts(call(eng), exp, name + ", no labels")
    total, cut = int(exp[2][0]), cc.cut_of(s)
    assert 0 < cut < total
    assert_contacts(call(eng, lab, total + 5), cc.expected(s, lab, total + 5, key="striped, every pair"), name + ", every pair")
    assert_contacts(call(eng, lab, total, True), cc.expected(s, lab, total, True, key="other body"), name + ", other_body")
    assert_contacts(call(eng, None, cut), cc.expected(s, None, cut, key="cut"), name + ", max_pairs %d" % cut)
    eng.destroy()


# 3
def test_pair_list_truncation_and_other_body(sb):
    import torch
    s = cc.big_scene(sb, "pile 4097 in 5000")
    maxp = s["buf"].max_particles
    eng = engine(sb, s)
    total = int(cc.expected(s, None, 0, key="plain")[2][0])
    every = cc.expected(s, None, total, key="all")[1]
    run = np.flatnonzero((every[1:, 0] == every[:-1, 0]) & (np.arange(1, total) > 1000))[0] + 1    # inside one particle's pairs
    assert every[run, 0] == every[run - 1, 0]
    for m in (0, 1, int(run), total, total + 7):
        exp = cref.contacts_ref(s["buf"], s["radius"], s["bounds"], None, m)
        if m == 0:
            assert_contacts(call(eng), exp, "no list")
            continue
        sentinel = torch.full((m + 3, 2), -77, dtype=torch.int32, device="cuda")
        touch, counts, pairs = eng.contacts(pairs=m, out=sentinel)
        assert rh.in_place(pairs, sentinel, (m, 2)) and (sentinel[m:] == -77).all()        # nothing at or behind max_pairs
        assert_contacts((touch.cpu().numpy(), sentinel[:m].cpu().numpy(), counts.cpu().numpy()), exp, "max_pairs %d" % m)
        if m == total + 7:
            assert (sentinel[total:m] == -1).all() and (sentinel[total - 1] >= 0).all()
    bl = eng.bodies(counts=False)[0]              # free particles: every particle its own body -> every pair is another body's
    stripes = cc.striped_labels(maxp)
    for labels, what in ((bl.cpu().numpy(), "bodies()"), (stripes, "stripes")):
        for m in (5, total):
            exp = cref.contacts_ref(s["buf"], s["radius"], s["bounds"], labels, m, True)
            assert_contacts(call(eng, labels, m, True), exp, "other_body, %s, %d" % (what, m))
    assert exp[2][1] < total and (exp[1][exp[2][1]:] == -1).all()
    eng.destroy()


# 4
PILE_GAP = 19.5       # between neighbouring blobs (2r = 20: they touch as uploaded, and the contact response acts from the first substep)


def pile_case(sb, mode):
    buf, bounds = sb.scenes.blob_pile_buffers(4, 3, gap=PILE_GAP)
    return dict(name="blob pile 4 x 3", buf=buf, bounds=bounds, radius=10.0, mode=sc.OFF if mode == OFF else sc.ALLPAIRS,
                program=[("frame", 2), ("step", 9), ("delete",)], compare_after=[-1, 0, 1, 2])


_pile_expected = {}


def pile_expected(sb, oracle, mode):
    case = pile_case(sb, mode)
    if case["mode"] not in _pile_expected:
        ref, out = sc.make_oracle(oracle, case), {}
        lab = cc.striped_labels(case["buf"].max_particles, 36)      # one label a blob

        def now():
            return cref.contacts_ref(ref.load_buffers(case["buf"].copy()), 10.0, case["bounds"], lab, 4000)
        out[-1] = now()
        for k, op in enumerate(case["program"]):
            sc.apply_to_oracle(ref, op)
            out[k] = now()
        _pile_expected[case["mode"]] = (out, lab)
    return case, _pile_expected[case["mode"]]


STEPPED = [(OFF, ATOMIC, {}), (ALLPAIRS, ATOMIC, {}), (GRID, ATOMIC, {}), (OFF, TILED, {}), (GRID, TILED, {}), (OFF, TILED, dict(block_substeps=1)),
           (GRID, TILED, dict(block_substeps=1))]


@pytest.mark.parametrize("mode,path,kw", STEPPED, ids=["mode %d path %d %s" % (m, p, "".join(k)) for m, p, k in STEPPED])
def test_settling_pile(sb, oracle, mode, path, kw):
    case, (exp, lab) = pile_expected(sb, oracle, mode)
    assert exp[-1][2][0] > 0 and exp[-1][2][2] > 0                                  # contacts between the blobs, and the floor
    assert mode == OFF or brief(exp[0][2]) != brief(exp[-1][2])                       # ... which the contact response changes
    eng = engine(sb, case, collision_mode=mode, path=path, **kw)
    assert_contacts(call(eng, lab, 4000), exp[-1], "pile, uploaded")
    for k, op in enumerate(case["program"]):
        sc.apply_to_engine(eng, op)
        assert_contacts(call(eng, lab, 4000), exp[k], "pile mode %d path %d, after op %d %s" % (mode, path, k, op[0]))
    eng.destroy()


# 5
@pytest.mark.parametrize("what,mk,kw", READ_ONLY, ids=[r[0] for r in READ_ONLY])
def test_read_only(sb, what, mk, kw):
    """frame, contacts, frame == frame, frame: the read-back byte for byte, the summary row, the promise flags, the schedule and
    the hash's counters; on the hybrid (a quiet lattice under SB_COLLIDE_GRID, blocked launches) the answer is the reference's on
    the engine's own read-back"""
    def calls(eng, case):
        got = eng.contacts(pairs=64)
        eng.contacts(labels=True, touch=False)
        eng.contacts_host(pairs=3)
        if what == "hybrid":
            exp = cref.contacts_ref(eng.load_buffers(case["buf"].copy()), 10.0, case["bounds"], None, 64)
            assert_contacts((got[0].cpu().numpy(), got[2].cpu().numpy(), got[1].cpu().numpy()), exp, "hybrid")

    def after(eng, case):
        if what == "tiled grid":
            assert eng.info("grid_builds") > 1      # across a rebuild of the hash
    rh.read_only(sb, what, mk, kw, engine, calls, keys=("grid_builds", "grid_cells", "grid_wide"), after=after)


# 6
def test_positions_at_the_calls_place_in_the_stream(sb):
    s = cc.big_scene(sb, "32 cells per side")
    eng = engine(sb, s)
    before = call(eng, None, 400)
    assert_contacts(before, cc.expected(s, None, 400, key="400"), "before")
    built = eng.info("contacts_table_build_us")
    D = s["D"]
    far = [int(d) for d in D if before[0][d, 0] == 0][:2]        # two particles that touch nobody
    t = eng.state_tensors()["particles"]
    t[far[1], 0:2] = t[far[0], 0:2]
    t[far[1], 0] += 3.0
    eng.write_particles_device(t)
    moved = s["buf"].copy()
    moved.particles[:, :2] = t[:, :2].cpu().numpy()
    exp = cref.contacts_ref(moved, s["radius"], s["bounds"], None, 400)
    got = call(eng, None, 400)
    assert_contacts(got, exp, "after the import")
    assert got[2][0] > before[2][0] and got[0][far[0], 0] >= 1 and sorted(far) in got[1].tolist()
    assert eng.info("contacts_table_build_us") == built       # no upload, no table build
    eng.destroy()


# 7
def test_every_combination_of_outputs_and_labels_true(sb):
    import torch
    case = pile_case(sb, GRID)
    buf = case["buf"]
    eng = engine(sb, case, collision_mode=GRID)
    maxp, m = buf.max_particles, 50
    bl = eng.bodies(counts=False)[0]
    exp = cref.contacts_ref(buf, 10.0, case["bounds"], bl.cpu().numpy(), m)
    assert exp[2][1] > 0 and exp[2][2] > 0                    # blobs touch each other, and the bottom course the floor
    for mask in range(1, 8):
        touch = torch.full((maxp + 2, 4), -77, dtype=torch.int32, device="cuda") if mask & 1 else False
        pairs = torch.full((m + 2, 2), -77, dtype=torch.int32, device="cuda") if mask & 2 else None
        counts = torch.full((6,), -77, dtype=torch.int64, device="cuda") if mask & 4 else False
        got = eng.contacts(labels=bl, touch=touch, counts=counts, pairs=m if mask & 2 else 0, out=pairs)
        assert got[0] is None if touch is False else rh.in_place(got[0], touch, (maxp, 4)), mask
        assert got[1] is None if counts is False else rh.in_place(got[1], counts, (4,)), mask
        assert len(got) == (3 if mask & 2 else 2)
        if mask & 1:
            assert np.array_equal(touch[:maxp].cpu().numpy(), exp[0]) and (touch[maxp:] == -77).all(), mask
        if mask & 2:
            assert rh.in_place(got[2], pairs, (m, 2)) and np.array_equal(pairs[:m].cpu().numpy(), exp[1]) and (pairs[m:] == -77).all(), mask
        if mask & 4:
            assert brief(counts[:4].cpu().numpy()) == brief(exp[2]) and (counts[4:] == -77).all(), mask
    # labels=True is bodies() first, on the same stream; torch's stream is ordered behind the call with no sync
    # (the side stream is a second engine's own, handed to torch: it goes away with that engine, where a stream taken from
    # torch's pool would stay for the life of the process)
    other = sb.Engine(bounds_size=1000.0, layout=2, max_particles=4, max_beams=4, collision_mode=OFF)
    side = torch.cuda.ExternalStream(other.stream(), device=torch.device("cuda", eng.device))
    with torch.cuda.stream(side):
        touch, counts, pairs = eng.contacts(labels=True, pairs=m)
        walled = (touch[:, 2] != 0).sum()
        got = (touch.clone(), pairs.clone(), counts.clone())
    side.synchronize()
    assert_contacts(tuple(x.cpu().numpy() for x in got), exp, "labels=True")
    assert int(walled) == exp[2][2] > 0
    host = eng.contacts_host(labels=bl.cpu().numpy(), pairs=m)
    assert host[0].dtype == np.int32 and host[1].dtype == np.int64 and host[2].dtype == np.int32
    assert_contacts((host[0], host[2], host[1]), exp, "host variant")
    del side
    other.destroy()
    eng.destroy()


def test_capacity_rows_beyond_the_highest_data_index(sb):
    """never stepped: empty, one particle, two particles that touch, at a capacity far above them"""
    import torch
    cap = 70000
    for pts, idx in (([], []), ([(10.0, 990.0)], [5]), ([(500.0, 300.0), (512.0, 300.0)], [69999, 3])):
        buf = sb.Buffers(2, cap, 4)
        for p, d in zip(pts, idx):
            buf.particles[d, :2] = p
        buf.mapping[:len(idx)] = idx
        buf.particle_count = len(idx)
        s = dict(buf=buf, bounds=1000.0, radius=10.0)
        eng = engine(sb, s)
        exp = cref.contacts_ref(buf, 10.0, 1000.0, None, 4)
        touch = torch.full((cap, 4), -77, dtype=torch.int32, device="cuda")
        t, c, p = eng.contacts(touch=touch, pairs=4)
        assert_contacts((t.cpu().numpy(), p.cpu().numpy(), c.cpu().numpy()), exp, "%d particles at capacity %d" % (len(idx), cap))
        assert brief(exp[2]) == ((0, -1, 0, 0), (0, -1, 1, 0), (1, -1, 0, 2))[len(idx)]
        if len(idx) == 1:
            assert t[5].tolist() == [0, -1, sb.engine.WALL_LEFT | sb.engine.WALL_HIGH, -1]
        eng.destroy()


# 8
def test_degenerate_geometry(sb):
    """a radius whose cell side is no ordinary number: all pairs at or below 4096 particles (only dist == 0 touches), refused above"""
    for n, ok in ((4096, True), (4097, False)):
        pts = np.zeros((n, 2), "f4")
        pts[:, 0] = 100.0 + 0.125 * (np.arange(n) // 2)       # two particles on every spot
        pts[:, 1] = 500.0
        buf, D = cc.free_scene(sb, n + 3, pts, seed=50)
        s = dict(buf=buf, bounds=1000.0, radius=1.0e-20)
        eng = engine(sb, s)
        if ok:
            assert eng.info("contacts_cells_per_side") == 1
            exp = cref.contacts_ref(buf, 1.0e-20, 1000.0, None, 3000)
            assert exp[2][0] == n // 2
            assert_contacts(call(eng, None, 3000), exp, "all pairs of %d" % n)
        else:
            with pytest.raises(sb.EngineError) as e:
                eng.contacts()
            assert e.value.status == 6      # SB_ERR_UNSUPPORTED
        eng.destroy()


def test_errors_on_a_live_engine(sb):
    import torch
    s = cc.big_scene(sb, "32 cells per side")
    buf = s["buf"]
    eng = sb.Engine(bounds_size=s["bounds"], layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=OFF)
    for f in (eng.contacts, eng.contacts_host):
        with pytest.raises(sb.EngineError) as e:
            f()
        assert e.value.status == 5          # SB_ERR_STATE
    eng.write_buffers(buf)
    mem = torch.empty(4 * buf.max_particles + 64, dtype=torch.int32, device="cuda")
    bad = (dict(touch=False, counts=False), dict(other_body=True), dict(touch=mem.data_ptr() + 2), dict(labels=mem.data_ptr() + 1),
           dict(counts=mem.data_ptr() + 4), dict(pairs=8, out=mem.data_ptr() + 2), dict(pairs=2 ** 31 + 1, out=mem.data_ptr()))
    for kw in bad:
        with pytest.raises(sb.EngineError) as e:
            eng.contacts(**kw)
        assert e.value.status == 1, kw      # SB_ERR_INVALID
    L, vp = sb.engine.load_library(), ctypes.c_void_p
    o = sb.engine.SbContactsOptions()
    size = ctypes.sizeof(o)
    for ssize, flags, pairs, reserved in ((size - 4, 0, 0, 0), (size + 8, 0, 0, 0), (size, 2, 0, 0), (size, 0, 0, 7), (size, 0, 5, 0)):
        o.struct_size, o.flags, o.max_pairs, o.reserved[3] = ssize, flags, pairs, reserved
        assert L.sb_contacts_device(eng._h, ctypes.byref(o), None, vp(mem.data_ptr()), None, None) == 1, (ssize, flags, pairs, reserved)
        host = np.empty((buf.max_particles, 4), np.int32)
        assert L.sb_contacts(eng._h, ctypes.byref(o), None, host.ctypes.data_as(vp), None, None) == 1, (ssize, flags, pairs, reserved)
    o.struct_size, o.flags, o.max_pairs, o.reserved[3] = 0, 2, 5, 7          # struct_size 0: all defaults, nothing else is read
    assert L.sb_contacts_device(eng._h, ctypes.byref(o), None, vp(mem.data_ptr()), None, None) == 0   # ... and the engine still works
    assert L.sb_contacts_device(eng._h, None, None, None, None, None) == 1
    d = [int(x) for x in s["D"][:4]]
    eng.halo_configure(d[:2], d[2:])
    with pytest.raises(sb.EngineError) as e:
        eng.contacts()
    assert e.value.status == 6          # SB_ERR_UNSUPPORTED
    eng.destroy()


def test_info_keys(sb):
    s = cc.big_scene(sb, "64 cells per side")
    eng = engine(sb, s)
    assert eng.info("contacts_kernel_scratch_bytes") == 0
    assert 0 < eng.info("contacts_kernel_vgprs") <= 64
    assert eng.info("contacts_table_build_us") == 0 and eng.info("contacts_cells_per_side") == 64
    eng.contacts()
    built = eng.info("contacts_table_build_us")
    assert built > 0
    eng.write_buffers(s["buf"])          # an upload drops the table
    eng.contacts()
    assert eng.info("grid_builds") == 0
    eng.destroy()


@needs_node
def test_node_contacts_equal_pythons(sb):
    r = run_node("contacts.gpu.test.js")
    assert r["ok"], r
    buf = sb.scenes.default_buffers(1, 128, 320)
    eng = sb.Engine(bounds_size=1000.0, particle_radius=10.0, subticks=64, layout=1, max_particles=128, max_beams=320,
                    collision_mode=GRID)
    eng.write_buffers(buf)
    eng.frame()
    touch, counts, pairs = eng.contacts_host(pairs=64)
    eng.destroy()
    assert r["touch"] == touch.reshape(-1).tolist(), json.dumps(r)
    assert r["pairs"] == pairs.reshape(-1).tolist()
    assert r["counts"] == [int(c) for c in counts] == r["secondCounts"] and counts[1] == -1
