"""Engine.summary() (sb_summary_device) against tests/batch_summary_ref.py on an oracle that ran the same program:
sums, means and counts by their bits, on every path; the same bytes however the reduction is cut; the batch's row for a scene
that fits a batch; reading changes nothing; torch's stream is ordered behind it."""
import json

import numpy as np
import pytest

import batch_cases as bc
import batch_harness as bh
import batch_summary_ref as sr
import report_harness as rh
import summary_cases as sc
from test_node_host import needs_node, run_node
from test_gpu_parity import ATOMIC, GRID, OFF, TILED, ALLPAIRS, assert_same

pytestmark = pytest.mark.gpu


def engine(sb, case, **kw):
    return rh.engine(sb, case["buf"], case["bounds"], **kw)


def check_now(eng, exp, what, partials=0):
    row, counts = eng.summary(counts=True, partials=partials)
    row, counts = row.cpu().numpy(), counts.cpu().numpy().astype(np.uint64)   # (torch's stream waits for the summary: no sync)
    print(what, "row", row.tolist(), "counts", counts.tolist())
    sr.assert_rows_equal(row, exp[0], what)
    assert np.array_equal(counts, exp[1]), "%s: counts %s, expected %s" % (what, counts, exp[1])
    return row


def run_case(sb, oracle, case, what, **kw):
    exp, _ = sc.expected(oracle, case)
    eng = engine(sb, case, **kw)
    if -1 in exp:
        check_now(eng, exp[-1], what + ", uploaded")
    for k, op in enumerate(case["program"]):
        sc.apply_to_engine(eng, op)
        if k in exp:
            check_now(eng, exp[k], "%s, after op %d %s" % (what, k, op[0]))
    eng.destroy()


# (every pair of collision mode and path the engine accepts: sb_create refuses SB_COLLIDE_ALLPAIRS on SB_PATH_TILED)
@pytest.mark.parametrize("mode,path", [(OFF, ATOMIC), (ALLPAIRS, ATOMIC), (GRID, ATOMIC), (OFF, TILED), (GRID, TILED)])
def test_default_scene(sb, oracle, mode, path):
    run_case(sb, oracle, sc.case_default(sb, sc.OFF if mode == OFF else sc.ALLPAIRS), "default, mode %d path %d" % (mode, path),
             collision_mode=mode, path=path)


def test_cut_independence(sb, oracle):
    case = sc.case_cut(sb)
    exp, _ = sc.expected(oracle, case)
    eng = engine(sb, case, collision_mode=OFF)
    for k in (-1, 0):
        if k == 0:
            sc.apply_to_engine(eng, case["program"][0])
        rows = [check_now(eng, exp[k], "cut %d, partials %d" % (k, m), partials=m) for m in (256, 1024, 16384, 0)]
        assert len({r.tobytes() for r in rows}) == 1
        assert eng.info("summary_partials") == 4096    # the engine's choice at W = 16384
    eng.destroy()


def test_capacity_far_above_the_scene(sb, oracle):
    run_case(sb, oracle, sc.case_capacity(sb), "capacity", collision_mode=OFF)


def test_where_the_default_cut_is_the_clamp(sb, oracle):
    """W = 2^21 for both trees: the engine's own cut is SB_SUMMARY_MAX_PARTIALS, not W / 4; that cut asked for, and the narrowest"""
    case = sc.case_clamp(sb)
    exp, _ = sc.expected(oracle, case)
    eng = engine(sb, case, collision_mode=OFF)
    for k in (-1, 0):
        if k == 0:
            sc.apply_to_engine(eng, case["program"][0])
        rows = [check_now(eng, exp[k], "clamp %d, partials %d" % (k, m), partials=m) for m in (262144, 256, 0)]
        assert len({r.tobytes() for r in rows}) == 1
        assert eng.info("summary_partials") == 262144 != sr.pow2_at_least(case["buf"].max_particles) // 4     # the default, run last
    eng.destroy()


@pytest.mark.parametrize("i", [0, 1, 2])
def test_tree_order_witness(sb, oracle, i):
    case = sc.witness_cases(sb)[i]
    run_case(sb, oracle, case, case["name"], collision_mode=OFF, path=ATOMIC)


def test_nonfinite(sb, oracle):
    run_case(sb, oracle, sc.case_nonfinite(sb), "non-finite", collision_mode=OFF, path=TILED)


@pytest.mark.parametrize("what,kw", [("tiled", dict(path=TILED, block_substeps=1)), ("blocked", dict(path=TILED)), ("atomic", dict(path=ATOMIC))])
def test_breaking_lattice(sb, oracle, what, kw):
    run_case(sb, oracle, sc.case_break(sb), "breaking, " + what, collision_mode=OFF, **kw)


def test_equals_the_batch(sb):
    """the heterogeneous scenes that fit a batch: same buffers, same constants, 2 frames each; words 0 .. 20 by their bits"""
    hc = bc.case_hetero(sb)
    consts = {op[1]: op[2] for op in hc["program"] if op[0] == "consts"}
    for i, buf in enumerate(hc["bufs"]):
        if buf is None:
            continue
        one = dict(hc, bufs=[buf])
        be = bh.make_batch(sb, one)
        bh.upload_each(be, [buf])
        bh.apply_to_batch(be, ("consts", 0, consts[i]))
        be.frame(2)
        brow = be.summary().cpu().numpy()[0]
        be.destroy()
        eng = sb.Engine(bounds_size=1000.0, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams,
                        collision_mode=GRID)
        eng.write_buffers(buf)
        eng.set_physics_constants(consts[i])
        eng.frame()
        eng.frame()
        erow = eng.summary().cpu().numpy()
        eng.destroy()
        print("scene", i, "engine", erow.tolist(), "batch", brow.tolist())
        assert erow[:21].tobytes() == brow[:21].tobytes(), "scene %d: engine %s, batch %s" % (i, erow, brow)


def word_for_word_scenes(sb):
    """(name, upload, pokes): the two scenes of zeros of both signs, the default scene at the batch's largest capacity, and the
    non-finite case's pokes on its scene as uploaded"""
    nf = sc.case_nonfinite(sb)
    return ([(c["name"], c["buf"], []) for c in sc.zero_sign_scenes(sb)] +
            [("default in 1024/4096", bc.fit(sb, sc.case_default(sb)["buf"], 1024, 4096), []), ("non-finite", nf["buf"], nf["program"][1][1])])


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_row_is_the_batchs_word_for_word(sb, i):
    """the same upload, not stepped, in an Engine and in a BatchEngine of one scene: all 24 words by their bits, NaN as NaN"""
    name, buf, pokes = word_for_word_scenes(sb)[i]
    be = bh.make_batch(sb, dict(layout=buf.layout, cap=(buf.max_particles, buf.max_beams), mode=0, bufs=[buf]))
    bh.upload_each(be, [buf])
    eng = sb.Engine(bounds_size=1000.0, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=OFF)
    eng.write_buffers(buf)
    if pokes:
        sc.apply_to_engine(eng, ("poke", pokes))
        p = be.state_tensors()[0]
        for d, col, v in pokes:
            p[0, d, col] = float(v)
        be.write_particles_device(p)
    brow, erow = be.summary().cpu().numpy()[0], eng.summary().cpu().numpy()
    be.destroy()
    eng.destroy()
    print(name, "engine", erow.view(np.uint32).tolist(), "batch", brow.view(np.uint32).tolist())
    assert erow[20] == 1.0 and erow[0] == buf.particle_count
    if pokes:
        assert erow[4] == 2                  # the poked particles are counted and left out
    sr.assert_rows_equal(erow, brow, name)


READ_ONLY = [("tiled grid", lambda sb: sc.case_break(sb), dict(collision_mode=GRID, path=TILED, tile_particles=256)),
             ("blocked", lambda sb: sc.case_break(sb), dict(collision_mode=OFF, path=TILED)),
             ("hybrid", None, dict(collision_mode=GRID))]


@pytest.mark.parametrize("what,mk,kw", READ_ONLY, ids=[r[0] for r in READ_ONLY])
def test_read_only(sb, what, mk, kw):
    """frame, summary, frame == frame, frame: the read-back byte for byte, and the promise flags and the schedule"""
    def calls(eng, case):
        eng.summary(counts=True)
        eng.summary(partials=256)
    rh.read_only(sb, what, mk, kw, engine, calls)


def test_ordering_and_host_variant(sb, oracle):
    """frame(), summary(), a torch reduction on another torch stream, no sync in between; summary_host() gives the same bytes"""
    import torch
    case = sc.case_default(sb)
    exp, _ = sc.expected(oracle, dict(case, program=[("frame", 1)], compare_after=[0]))
    eng = engine(sb, case, collision_mode=GRID)
    side = torch.cuda.Stream(device=torch.device("cuda", eng.device))
    with torch.cuda.stream(side):
        eng.frame()
        row = eng.summary()
        k = torch.argmax(row[10:14])
        got = row.clone()
    side.synchronize()
    sr.assert_rows_equal(got.cpu().numpy(), exp[0][0], "ordering")
    assert int(k) == int(np.argmax(exp[0][0][10:14]))
    hrow, hcounts = eng.summary_host()
    assert hrow.tobytes() == got.cpu().numpy().tobytes() and np.array_equal(hcounts, exp[0][1])
    eng.destroy()


def test_errors_on_a_live_engine(sb):
    import torch
    case = sc.case_default(sb)
    buf = case["buf"]
    eng = sb.Engine(bounds_size=1000.0, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=OFF)
    with pytest.raises(sb.EngineError) as e:
        eng.summary()
    assert e.value.status == 5          # SB_ERR_STATE
    eng.write_buffers(buf)
    for bad in (1, 255, 257, 300, 1 << 19):
        with pytest.raises(sb.EngineError) as e:
            eng.summary(partials=bad)
        assert e.value.status == 1      # SB_ERR_INVALID
    row = torch.empty(32, dtype=torch.float32, device="cuda")
    with pytest.raises(sb.EngineError) as e:
        eng.summary(out=row.data_ptr() + 2)
    assert e.value.status == 1
    with pytest.raises(sb.EngineError) as e:
        eng.summary(out=row, counts=row.data_ptr() + 4)
    assert e.value.status == 1
    import ctypes
    L, vp = sb.engine.load_library(), ctypes.c_void_p
    o = sb.engine.SbSummaryOptions()
    for size, reserved in ((ctypes.sizeof(o) - 4, 0), (ctypes.sizeof(o) + 8, 0), (ctypes.sizeof(o), 7)):
        o.struct_size, o.partials, o.reserved[5] = size, 0, reserved
        assert L.sb_summary_device(eng._h, ctypes.byref(o), vp(row.data_ptr()), None) == 1, (size, reserved)
        assert L.sb_summary(eng._h, ctypes.byref(o), vp(row.data_ptr()), None) == 1, (size, reserved)
    assert L.sb_summary_device(eng._h, None, None, None) == 1                      # a NULL row
    eng.summary(out=row)                # ... and the engine still works
    eng.halo_configure([0, 1], [2, 3])
    with pytest.raises(sb.EngineError) as e:
        eng.summary()
    assert e.value.status == 6          # SB_ERR_UNSUPPORTED
    eng.destroy()


def test_kernels_use_no_scratch(sb):
    """0 spilled registers means no scratch; 256 VGPRs is where a kernel of 256 threads drops to one wave per SIMD (the deepest leaf
    kernel, 16 leaves a thread with all their loads in flight, has 184)"""
    case = sc.case_default(sb)
    eng = engine(sb, case, collision_mode=OFF)
    assert eng.info("summary_kernel_scratch_bytes") == 0
    assert 0 < eng.info("summary_kernel_vgprs") <= 256
    eng.summary()
    assert eng.info("summary_table_build_us") > 0 and eng.info("summary_partials") == 256
    eng.destroy()


@needs_node
def test_node_summary_equals_pythons(sb):
    r = run_node("summary.gpu.test.js")
    assert r["ok"], r
    buf = sb.scenes.default_buffers(1, 128, 320)
    eng = sb.Engine(bounds_size=1000.0, particle_radius=10.0, subticks=64, layout=1, max_particles=128, max_beams=320,
                    collision_mode=OFF)
    eng.write_buffers(buf)
    eng.frame()
    row, counts = eng.summary_host()
    eng.destroy()
    assert r["row"] == row.view(np.uint32).tolist(), json.dumps(r)
    assert r["counts"] == [int(c) for c in counts] == r["workerCounts"]
