"""Engine.bodies() (sb_bodies_device) against tests/batch_bodies_ref.py's bodies_ref on what the load_buffers of an
oracle that ran the same program returns: labels, sizes and counts by value, on every path; graphs far beyond one workgroup with
every mapping shuffled; every combination of outputs; liveness read on the device; the batch's answer for a scene that fits a
batch; reading changes nothing; torch's stream is ordered behind it."""
import ctypes
import json

import numpy as np
import pytest

import batch_bodies_ref as br
import batch_cases as bcs
import batch_harness as bh
import bodies_cases as bc
import report_harness as rh
import summary_cases as sc
from test_gpu_parity import ATOMIC, GRID, OFF, TILED, ALLPAIRS, assert_same
from test_gpu_summary import READ_ONLY
from test_node_host import needs_node, run_node

pytestmark = pytest.mark.gpu


def engine(sb, case, **kw):
    return rh.engine(sb, case["buf"], case["bounds"], **kw)


def brief(counts):
    return tuple(int(x) for x in counts)


def assert_bodies(got, exp, what):
    """(labels, sizes, counts) by value; counts as the same four integers"""
    labels, sizes, counts = (np.asarray(x) for x in got)
    print(what, "counts", brief(counts), "expected", brief(exp[2]))
    assert brief(counts) == brief(exp[2]), "%s: counts %s, expected %s" % (what, brief(counts), brief(exp[2]))
    bad = np.flatnonzero(labels != exp[0])
    assert bad.size == 0, "%s: %d labels differ, first at data index %d: %d, expected %d" % (what, bad.size, bad[0], labels[bad[0]], exp[0][bad[0]])
    bad = np.flatnonzero((sizes != exp[1]).any(axis=1))
    assert bad.size == 0, "%s: %d size rows differ, first %d: %s, expected %s" % (what, bad.size, bad[0], sizes[bad[0]], exp[1][bad[0]])


def check_now(eng, exp, what):
    labels, counts, sizes = eng.bodies(sizes=True)
    assert counts.dtype.is_signed and counts.element_size() == 8 and labels.element_size() == 4
    got = (labels.cpu().numpy(), sizes.cpu().numpy(), counts.cpu().numpy())   # (torch's stream waits for the call: no sync)
    assert_bodies(got, exp, what)
    return got


def run_case(sb, oracle, case, what, **kw):
    exp = bc.expected_cached(oracle, case)
    eng = engine(sb, case, **kw)
    out = {}
    if -1 in exp:
        out[-1] = check_now(eng, exp[-1], what + ", uploaded")
    for k, op in enumerate(case["program"]):
        sc.apply_to_engine(eng, op)
        if k in exp:
            out[k] = check_now(eng, exp[k], "%s, after op %d %s" % (what, k, op[0]))
    eng.destroy()
    return out


# 1 (every pair of collision mode and path the engine accepts: tests/test_gpu_summary.py's five)
@pytest.mark.parametrize("mode,path", [(OFF, ATOMIC), (ALLPAIRS, ATOMIC), (GRID, ATOMIC), (OFF, TILED), (GRID, TILED)])
def test_default_scene(sb, oracle, mode, path):
    run_case(sb, oracle, bc.case_default(sb, sc.OFF if mode == OFF else sc.ALLPAIRS), "default, mode %d path %d" % (mode, path),
             collision_mode=mode, path=path)


# 2
PATHS = [("tiled", dict(path=TILED, block_substeps=1)), ("blocked", dict(path=TILED)), ("atomic", dict(path=ATOMIC))]


@pytest.mark.parametrize("what,kw", PATHS, ids=[p[0] for p in PATHS])
def test_breaking_lattice(sb, oracle, what, kw):
    """summary_cases.case_break: one body while the flags of substep 40 are pending; the delete pass takes their beams out of the
    sizes; the frame after leaves pieces (what the oracle says of each point: tests/test_bodies_cpu.py)"""
    out = run_case(sb, oracle, bc.case_break(sb), "breaking, " + what, collision_mode=OFF, **kw)
    assert brief(out[0][2]) == (1, 144, 0, 0) and out[1][1][0, 1] < out[0][1][0, 1] and out[2][2][0] > 1


@pytest.mark.parametrize("what,kw", PATHS, ids=[p[0] for p in PATHS])
def test_breaking_lattice_apart_by_the_delete_pass(sb, oracle, what, kw):
    out = run_case(sb, oracle, bc.case_break_apart(sb), "apart, " + what, collision_mode=OFF, **kw)
    assert brief(out[0][2]) == (1, 144, 0, 0) and out[1][2][0] > 1


# 3
@pytest.mark.parametrize("path", [None, ATOMIC], ids=["default", "atomic"])
@pytest.mark.parametrize("name", list(bc.GRAPHS))
def test_graphs_beyond_one_workgroup(sb, oracle, name, path):
    case = bc.graph_case(sb, name)
    kw = {} if path is None else dict(path=path)
    try:
        eng = engine(sb, case, collision_mode=OFF, **kw)
    except sb.EngineError as e:
        if name.startswith("star") and path is None:
            pytest.skip("the default path's upload refuses the star: %s" % e)
        raise
    exp = bc.expected_cached(oracle, case)[-1]
    got = check_now(eng, exp, "%s, %s path" % (name, "default" if path is None else "atomic"))
    assert brief(got[2]) == case["counts"]
    eng.destroy()


# 4
def test_capacity_far_above_the_scene(sb, oracle):
    case = bc.case_capacity(sb)
    out = run_case(sb, oracle, case, "capacity", collision_mode=OFF)
    buf = case["buf"]
    lives = np.zeros(buf.max_particles, bool)
    lives[buf.mapping[:buf.particle_count].astype(np.int64)] = True
    for labels, sizes, counts in out.values():
        assert np.array_equal(labels == -1, ~lives)
        assert not sizes[np.arange(buf.max_particles) != counts[3]].any() and sizes[counts[3]].tolist() == [48, buf.beam_count]


# 5
def test_every_combination_of_outputs(sb, oracle):
    import torch
    case = bc.case_default(sb)
    exp = bc.expected_cached(oracle, case)[-1]
    eng = engine(sb, case, collision_mode=OFF)
    maxp = case["buf"].max_particles
    seen = []
    for mask in range(1, 8):
        labels = torch.full((maxp,), -77, dtype=torch.int32, device="cuda") if mask & 1 else False
        sizes = torch.full((maxp, 2), -77, dtype=torch.int32, device="cuda") if mask & 2 else False
        counts = torch.full((4,), -77, dtype=torch.int64, device="cuda") if mask & 4 else False
        got = eng.bodies(labels=labels, sizes=sizes, counts=counts)
        assert got[0] is (labels if mask & 1 else None) and got[1] is (counts if mask & 4 else None)
        assert len(got) == (3 if mask & 2 else 2) and (not mask & 2 or got[2] is sizes)
        if mask & 1:
            assert np.array_equal(labels.cpu().numpy(), exp[0]), mask
        if mask & 2:
            assert np.array_equal(sizes.cpu().numpy(), exp[1]), mask
        if mask & 4:
            assert brief(counts.cpu().numpy()) == brief(exp[2]), mask
            seen.append(brief(counts.cpu().numpy()))
    assert len(seen) == 4 and len(set(seen)) == 1       # counts alone (sizes in the engine's scratch) == counts beside sizes
    eng.destroy()


# 6
@pytest.mark.parametrize("what,kw", PATHS, ids=[p[0] for p in PATHS])
def test_upload_that_removed_beams(sb, what, kw):
    whole, cut = bc.cut_lattice(sb)
    eng = sb.Engine(bounds_size=1000.0, layout=2, max_particles=whole.max_particles, max_beams=whole.max_beams, collision_mode=OFF, **kw)
    eng.write_buffers(whole)
    assert_bodies(eng.bodies_host(), br.bodies_ref(whole), what + ", whole")
    eng.write_buffers(cut)
    assert eng.info("uploads_edited") == 1 and eng.info("substeps_done") == 0
    got = eng.bodies_host()
    assert_bodies(got, br.bodies_ref(cut), what + ", cut")
    assert brief(got[2]) == (2, 144, 0, 0)              # two bodies, and no delete pass has run
    eng.destroy()


# 7
def test_liveness_is_read_on_the_device(sb, oracle):
    case = bc.case_break_apart(sb)
    exp = bc.expected_cached(oracle, case)
    eng = engine(sb, case, collision_mode=OFF)
    eng.step(bc.APART_STEPS)
    assert eng.summary(counts=True)[1][3].item() > 0    # flags are pending
    first = check_now(eng, exp[0], "flags pending")
    eng.delete_pass()                                   # no upload, no table build in between
    built = eng.info("bodies_table_build_us")
    second = check_now(eng, exp[1], "after the delete pass")
    assert eng.info("bodies_table_build_us") == built
    assert brief(first[2]) == (1, 144, 0, 0) and second[2][0] > 1 and second[1][:, 1].sum() < first[1][:, 1].sum()
    eng.destroy()


# 8
@pytest.mark.parametrize("which", ["default", "breaking"])
def test_equals_the_batch(sb, which):
    if which == "default":
        case = dict(bcs.case_default(sb, 1), program=[("frame", 2), ("step", 5)])
    else:
        c = bcs.case_break(sb)
        case = dict(c, bufs=[c["bufs"][2]], program=[("step", bc.APART_STEPS), ("delete",), ("frame", 1)])
    buf = case["bufs"][0]
    be = bh.make_batch(sb, case)
    bh.upload_each(be, [buf])
    eng = sb.Engine(bounds_size=1000.0, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams,
                    collision_mode=GRID if case["mode"] else OFF)
    eng.write_buffers(buf)
    pieces = []
    for k, op in enumerate([None] + case["program"]):
        if op is not None:
            bh.apply_to_batch(be, op)
            sc.apply_to_engine(eng, op)
        bl, bcnt, bs = be.bodies(sizes=True)
        el, ecnt, es = eng.bodies(sizes=True)
        exp = (bl.cpu().numpy()[0], bs.cpu().numpy()[0], bcnt.cpu().numpy()[0])
        assert_bodies((el.cpu().numpy(), es.cpu().numpy(), ecnt.cpu().numpy()), exp, "%s, op %d" % (which, k))
        pieces.append(int(ecnt[0]))
    be.destroy()
    eng.destroy()
    assert pieces[0] == (9 if which == "default" else 1) and (which == "default" or pieces[-1] > 1)


# 9
@pytest.mark.parametrize("what,mk,kw", READ_ONLY, ids=[r[0] for r in READ_ONLY])
def test_read_only(sb, what, mk, kw):
    """frame, bodies, frame == frame, frame: the read-back byte for byte, the summary row, the promise flags and the schedule"""
    def calls(eng, case):
        eng.bodies(sizes=True)
        eng.bodies(labels=False)
        eng.bodies_host()
    rh.read_only(sb, what, mk, kw, engine, calls)


# 10
def test_ordering_and_host_variant(sb, oracle):
    """frame(), bodies(), a torch reduction on another torch stream, no sync in between; bodies_host() gives the same"""
    import torch
    case = bc.case_default(sb)
    exp = bc.expected_cached(oracle, case)[0]           # after 2 frames
    eng = engine(sb, case, collision_mode=GRID)
    side = torch.cuda.Stream(device=torch.device("cuda", eng.device))
    with torch.cuda.stream(side):
        eng.frame()
        eng.frame()
        labels, counts, sizes = eng.bodies(sizes=True)
        per_body = torch.zeros(case["buf"].max_particles, dtype=torch.int32, device=labels.device)
        live = labels >= 0
        per_body.index_add_(0, labels[live].long(), torch.ones(int(live.sum()), dtype=torch.int32, device=labels.device))
        got = (labels.clone(), sizes.clone(), counts.clone())
    side.synchronize()
    assert_bodies(tuple(x.cpu().numpy() for x in got), exp, "ordering")
    assert np.array_equal(per_body.cpu().numpy(), exp[1][:, 0])
    host = eng.bodies_host()
    assert host[0].dtype == np.int32 and host[1].dtype == np.int32 and host[2].dtype == np.int64
    assert_bodies(host, exp, "host variant")
    eng.destroy()


# 11
def test_errors_on_a_live_engine(sb):
    import torch
    case = bc.case_default(sb)
    buf = case["buf"]
    eng = sb.Engine(bounds_size=1000.0, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=OFF)
    with pytest.raises(sb.EngineError) as e:
        eng.bodies()
    assert e.value.status == 5          # SB_ERR_STATE
    with pytest.raises(sb.EngineError) as e:
        eng.bodies_host()
    assert e.value.status == 5
    eng.write_buffers(buf)
    with pytest.raises(sb.EngineError) as e:
        eng.bodies(labels=False, sizes=False, counts=False)
    assert e.value.status == 1          # SB_ERR_INVALID: three NULL outputs
    mem = torch.empty(4 * buf.max_particles, dtype=torch.int32, device="cuda")
    for kw in (dict(labels=mem.data_ptr() + 2), dict(labels=False, sizes=mem.data_ptr() + 1), dict(labels=False, counts=mem.data_ptr() + 4)):
        with pytest.raises(sb.EngineError) as e:
            eng.bodies(**kw)
        assert e.value.status == 1, kw
    L, vp = sb.engine.load_library(), ctypes.c_void_p
    o = sb.engine.SbBodiesOptions()
    for size, reserved in ((ctypes.sizeof(o) - 4, 0), (ctypes.sizeof(o) + 8, 0), (ctypes.sizeof(o), 7)):
        o.struct_size, o.reserved[6] = size, reserved
        assert L.sb_bodies_device(eng._h, ctypes.byref(o), vp(mem.data_ptr()), None, None) == 1, (size, reserved)
        host = np.empty(buf.max_particles, np.int32)
        assert L.sb_bodies(eng._h, ctypes.byref(o), host.ctypes.data_as(vp), None, None) == 1, (size, reserved)
    o.struct_size, o.reserved[6] = ctypes.sizeof(o), 0
    assert L.sb_bodies_device(eng._h, ctypes.byref(o), vp(mem.data_ptr()), None, None) == 0   # ... and the engine still works
    assert L.sb_bodies_device(eng._h, None, None, None, None) == 1
    eng.halo_configure([0, 1], [2, 3])
    with pytest.raises(sb.EngineError) as e:
        eng.bodies()
    assert e.value.status == 6          # SB_ERR_UNSUPPORTED
    eng.destroy()


# 12
def test_kernels_use_no_scratch(sb):
    case = bc.case_default(sb)
    eng = engine(sb, case, collision_mode=OFF)
    assert eng.info("bodies_kernel_scratch_bytes") == 0
    assert 0 < eng.info("bodies_kernel_vgprs") <= 64
    assert eng.info("bodies_table_build_us") == 0
    eng.bodies()
    assert eng.info("bodies_table_build_us") > 0
    eng.destroy()


# 13
@needs_node
def test_node_bodies_equal_pythons(sb):
    r = run_node("bodies.gpu.test.js")
    assert r["ok"], r
    buf = sb.scenes.default_buffers(1, 128, 320)
    eng = sb.Engine(bounds_size=1000.0, particle_radius=10.0, subticks=64, layout=1, max_particles=128, max_beams=320,
                    collision_mode=OFF)
    eng.write_buffers(buf)
    eng.frame()
    labels, _, counts = eng.bodies_host()
    eng.destroy()
    assert r["labels"] == labels.tolist(), json.dumps(r)
    assert r["counts"] == [int(c) for c in counts] == r["secondCounts"] and counts[0] == 9
