"""Engine.body_summary() (sb_body_summary_device) against tests/body_summary_ref.py -- the dense restatement of the
definition -- on the engine's own read-back (and, for pending flags, on an oracle that ran the same program): rows, exact counts
and ranks by their bits, no tolerance anywhere.  Scenes live in tests/body_summary_cases.py; tests/test_body_summary_cpu.py pins
what they must show on the CPU."""
import ctypes

import numpy as np
import pytest

import batch_body_summary_ref as qr
import batch_cases as bcs
import batch_harness as bh
import bodies_cases as bc
import body_summary_cases as yc
import body_summary_ref as yr
import report_harness as rh
import summary_cases as sc
from test_gpu_parity import ATOMIC, GRID, OFF, TILED, assert_same
from test_gpu_summary import READ_ONLY
from test_node_host import needs_node, run_node

pytestmark = pytest.mark.gpu

SENTINEL = -77


def engine(sb, buf, bounds=None, **kw):
    kw.setdefault("collision_mode", OFF)
    return rh.engine(sb, buf, bounds or bc.bounds_of(max(buf.particle_count, 1)), **kw)


def call(eng, rows, labels=None):
    """(rows, counts, rank) as numpy arrays; labels: None (the engine's bodies) or a numpy array [maxP] of the caller's"""
    import torch
    r, c, k = eng.body_summary(None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, np.int32)).cuda(), rows=rows,
                               counts=True, rank=True)
    assert tuple(r.shape) == (rows, 24) and tuple(c.shape) == (rows, 8) and tuple(k.shape) == (eng.max_particles,)
    return r.cpu().numpy(), c.cpu().numpy(), k.cpu().numpy()   # (torch's stream waits for the call: no sync)


def check(eng, now, rows, labels=None, pending=None, what=""):
    """the call against the reference on `now` (the scene as read back); with labels None the groups are the bodies of `now`"""
    got = call(eng, rows, labels)
    exp = yr.body_summary_ref(now, yc.body_labels(now) if labels is None else labels, rows, pending)
    print(what, "rows", rows, "counts", got[1][:3].tolist())
    yr.assert_equal(got, exp, what)
    return got


# 1
@pytest.mark.parametrize("name", list(yc.SMALL))
def test_basic_and_edge_scenes(sb, name):
    buf = yc.scene(sb, name)
    eng = engine(sb, buf, path=ATOMIC)
    for m in (1, min(3, buf.max_particles), buf.max_particles):
        got = check(eng, buf, m, what="%s, %d rows" % (name, m))
    assert got[1][:, 0].sum() == buf.particle_count == (got[2] >= 0).sum()
    if name == "no particles":
        assert (got[1] == np.array(yr.EMPTY_COUNTS)).all() and (got[2] == -1).all()
    eng.destroy()


# 2
@pytest.mark.parametrize("name", list(yc.BIG))
def test_past_a_batch_and_past_one_workgroup(sb, name):
    buf = yc.scene(sb, name)
    eng = engine(sb, buf, path=ATOMIC)
    got = check(eng, buf, 8, what=name)
    groups = len(np.unique(yc.body_labels(buf)[yc.body_labels(buf) >= 0]))
    assert got[2].max() == groups - 1 and (got[2] >= 0).sum() == buf.particle_count
    if name.startswith("16 pieces"):
        assert (got[1][:, 0] == 256).all() and (np.diff(got[1][:, 2]) > 0).all()     # a tie: the label decides
    if name.startswith("shuffled"):
        assert groups > 20000
    eng.destroy()


# 3 (yc.SORT_KEYS = yc.SCAN_WORDS = 1024 groups fill one block of the group sort and of the scan of its counts)
@pytest.mark.parametrize("name", list(yc.EDGES))
def test_group_counts_at_the_block_edges(sb, name):
    buf = yc.scene(sb, name)
    eng = engine(sb, buf, path=ATOMIC)
    n = buf.particle_count
    got = check(eng, buf, 8, what=name)
    rank = got[2]
    lives = np.sort(buf.mapping[:n].astype(np.int64))
    assert np.array_equal(rank[lives], np.arange(n))          # every group one particle: the rank is the order of the labels
    full = call(eng, buf.max_particles)
    assert (full[1][:n, 0] == 1).all() and (full[1][n:] == np.array(yr.EMPTY_COUNTS)).all() and np.array_equal(full[1][:n, 2], lives)
    eng.destroy()


# 3b (tests/test_body_summary_cpu.py shows, on the CPU, what each run reaches and that a scan without its carry gives other words)
PAST_RUNS = [("sparse up to index 2^20+", None), ("sparse up to index 2^20+", "stripes"), ("sparse up to index 2^20+", "uneven"),
             ("sparse in capacity 2^21 + 1", "stripes"), ("2^18 + 1025 particles, pairs and singles", None),
             ("2^18 + 1025 particles, pairs and singles", "bodies, some outside")]


@pytest.mark.parametrize("name,which", PAST_RUNS, ids=["%s, %s" % r for r in PAST_RUNS])
def test_past_256_scan_blocks(sb, name, which):
    """more than 256 blocks in the scan of a sort's digit counts (Wn = 2^21) and in the scan of the head flags (Wn = 2^19): the
    second iteration of the loop over the block sums, with its carry"""
    buf = yc.scene(sb, name)
    labels = None if which is None else yc.caller_labels(buf, which)
    eng = engine(sb, buf, path=ATOMIC)
    for m in (1, 8, buf.max_particles):
        got = check(eng, buf, m, labels, what="%s, %s, %d rows" % (name, which, m))
    assert (got[2] >= 0).sum() == got[1][:, 0].sum() <= buf.particle_count
    again = call(eng, buf.max_particles, labels)
    assert tuple(g.tobytes() for g in again) == tuple(g.tobytes() for g in got)     # two calls in a row: identical bytes
    eng.destroy()


# 4
def test_capacity_far_above_the_scene_and_the_same_scene_tight(sb):
    wide, tight = yc.sparse_in_big_capacity(sb)
    out = {}
    for k, buf in (("wide", wide), ("tight", tight)):
        eng = engine(sb, buf, bounds=2000.0)
        stripes = yc.caller_labels(buf, "stripes")
        out[k] = (check(eng, buf, 2, what=k), check(eng, buf, 5, stripes, what=k + ", stripes"))
        if k == "wide":
            assert eng.info("body_summary_scratch_bytes") < 64 * buf.max_particles    # by the highest index in use, not the capacity
        eng.destroy()
    # what the definition says of the two: W differs (2^20 against 2^11), so the sums need not agree; everything order-free does
    a, b = out["wide"][0], out["tight"][0]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2][:tight.max_particles], b[2])
    for w in qr.EXTREME_WORDS:
        assert a[0][:, w].tobytes() == b[0][:, w].tobytes(), w


# 5
@pytest.mark.parametrize("which", ["default", "lattice"])
def test_equals_the_batch_after_two_frames(sb, which):
    if which == "default":
        buf, mode = sb.scenes.default_buffers(1, 128, 320), 1
    else:
        buf, mode = yc.with_velocities(bcs.fit(sb, sb.scenes.lattice_buffers(32, 32, d=30.0, origin=(40.0, 40.0), layout=2), 1024, 4096), 3), 0
    case = dict(layout=buf.layout, cap=(buf.max_particles, buf.max_beams), mode=mode, bufs=[buf])
    be = bh.make_batch(sb, case)
    bh.upload_each(be, [buf])
    eng = engine(sb, buf, bounds=1000.0, collision_mode=GRID if mode else OFF)
    be.frame(2)
    eng.frame()
    eng.frame()
    for m in (1, 16):
        brow, brank = be.body_summary(rows=m, rank=True)
        got = call(eng, m)
        qr.assert_equal((got[0], got[2]), (brow.cpu().numpy()[0], brank.cpu().numpy()[0]), "%s, %d rows" % (which, m))
        assert np.array_equal(got[1][:, :6].astype(np.float32), got[0][:, :6])
    be.destroy()
    eng.destroy()


@pytest.mark.parametrize("which", ["default", "zeros"])
def test_rows_and_ranks_are_the_batchs_word_for_word(sb, which):
    """the same upload and the same labels, not stepped, in an Engine and in a BatchEngine of one scene: every word of the rows
    (NaN as NaN) and every rank by its bits -- the default scene at the batch's capacity with its own bodies, and the zeros of
    both signs at data indices 0 and 256 as one group (min -0.0, max +0.0)"""
    if which == "default":
        buf = bcs.fit(sb, bc.case_default(sb)["buf"], 1024, 4096)
        labels = yc.body_labels(buf)
    else:
        buf = sc.zero_sign_scenes(sb)[0]["buf"]
        labels = np.zeros(buf.max_particles, np.int32)
    labels = np.ascontiguousarray(labels, np.int32)
    be = bh.make_batch(sb, dict(layout=buf.layout, cap=(buf.max_particles, buf.max_beams), mode=0, bufs=[buf]))
    bh.upload_each(be, [buf])
    eng = engine(sb, buf, bounds=1000.0)
    import torch
    for m in (1, 16):
        brow, brank = be.body_summary(torch.from_numpy(labels[None, :].copy()).cuda(), rows=m, rank=True)
        got = call(eng, m, labels)
        brow, brank = brow.cpu().numpy()[0], brank.cpu().numpy()[0]
        print(which, m, "engine", got[0][0].view(np.uint32).tolist(), "batch", brow[0].view(np.uint32).tolist())
        qr.assert_equal((got[0], got[2]), (brow, brank), "%s, %d rows" % (which, m))
    if which == "zeros":
        bits = got[0][0].view(np.uint32)
        assert got[1][0, 0] == 2 and bits[10] == bits[11] == 0x80000000 and bits[12] == bits[13] == 0
    be.destroy()
    eng.destroy()


# 6
@pytest.mark.parametrize("which", ["lattice", "breaking"])
def test_one_body_is_the_summary_row_by_bits(sb, which):
    if which == "lattice":
        buf = yc.with_velocities(sb.scenes.lattice_buffers(40, 30, d=30.0, origin=(100.0, 100.0), layout=2), 5)
        eng = engine(sb, buf, bounds=2000.0)
        eng.step(7)
    else:
        buf = sc.case_break(sb)["buf"]
        eng = engine(sb, buf, bounds=1000.0)
        eng.step(sc.BREAK_STEPS)
    row, counts = eng.summary(counts=True)
    row, counts = row.cpu().numpy(), counts.cpu().numpy()
    got = call(eng, 2)
    assert got[1][0, 0] == buf.particle_count and got[1][1, 2] == -1          # one body
    w = list(yr.SUMMARY_SHARED_WORDS)
    assert got[0][0, w].tobytes() == row[w].tobytes(), (got[0][0].tolist(), row.tolist())
    assert got[1][0, [0, 1, 3, 4, 5]].tolist() == [int(counts[k]) for k in (0, 1, 3, 4, 5)]
    if which == "breaking":
        assert got[1][0, 3] > 0      # flags are pending
    eng.destroy()


# 7
def test_liveness_is_read_on_the_device(sb, oracle):
    case = bc.case_break_apart(sb)
    buf = case["buf"]
    ref = sc.make_oracle(oracle, case)
    eng = engine(sb, buf, bounds=1000.0)
    eng.step(bc.APART_STEPS)
    sc.apply_to_oracle(ref, case["program"][0])
    now = eng.load_buffers(buf.copy())
    first = check(eng, now, 8, pending=qr.pending_slots_of(ref, buf), what="flags pending")
    built = eng.info("body_summary_table_build_us")
    eng.delete_pass()                                    # no upload, no table build in between
    second = check(eng, eng.load_buffers(buf.copy()), 8, what="after the delete pass")
    assert eng.info("body_summary_table_build_us") == built > 0
    assert first[1][0, 0] == 144 and first[1][0, 3] > 0 and first[1][1, 2] == -1
    assert second[1][1, 2] >= 0 and second[1][:, 3].sum() == 0 and second[1][:, 1].sum() < first[1][0, 1]
    eng.destroy()


# 8
def test_cut_lattice_after_a_plan_keeping_upload(sb):
    whole, cut = bc.cut_lattice(sb)
    eng = engine(sb, whole, bounds=1000.0)
    check(eng, whole, 4, what="whole")
    eng.write_buffers(cut)
    assert eng.info("uploads_edited") == 1
    got = check(eng, cut, 4, what="cut")
    assert got[1][:3, 0].tolist() == [144, 144, 0] and got[1][0, 2] < got[1][1, 2]
    eng.destroy()


# 9
@pytest.mark.parametrize("which", ["stripes", "outside", "split"])
def test_callers_labels(sb, which):
    buf = yc.scene(sb, "path 4097")
    eng = engine(sb, buf, path=ATOMIC)
    lab = yc.caller_labels(buf, which)
    got = check(eng, buf, 8, lab, what=which)
    if which == "outside":
        assert got[1][0, 2] == buf.max_particles - 1 and got[1][1, 2] == -1 and 0 < got[1][0, 0] < buf.particle_count and (got[2] == -1).sum() > 2000
    if which == "split":
        assert got[1][:2, 1].sum() < buf.beam_count      # beams across the halves belong to no group
    eng.destroy()


# 10
def test_nonfinite_particles_and_row_counts(sb):
    import torch
    case = sc.case_default(sb, sc.OFF)
    buf = case["buf"]
    eng = engine(sb, buf, bounds=1000.0)
    eng.frame()
    t = eng.state_tensors()["particles"]
    t[7, 0], t[40, 3] = float("nan"), float("inf")
    eng.write_particles_device(t)
    now = eng.load_buffers(buf.copy())
    groups = 9
    for m in (1, groups - 1, buf.max_particles):
        got = check(eng, now, m, what="non-finite, %d rows" % m)
    rows, counts, rank = got
    assert counts[:, 4].sum() == 2 and counts[groups, 2] == -1 and counts[groups - 1, 2] >= 0
    # rank against the exact counts: the particles of rank k are row k's
    assert np.array_equal(np.bincount(rank[rank >= 0], minlength=groups), counts[:groups, 0])
    assert call(eng, groups - 1)[2].max() == groups - 1      # the rank still names the cut row
    # ... and the counts add up to summary()'s
    total = eng.summary(counts=True)[1].cpu().numpy()
    assert [int(counts[:, k].sum()) for k in (0, 1, 3, 4, 5)] == [int(total[k]) for k in (0, 1, 3, 4, 5)]
    eng.destroy()


# 11
def test_every_combination_of_outputs_and_two_calls_in_a_row(sb):
    import torch
    buf = yc.scene(sb, "16 pieces of 256")
    eng = engine(sb, buf, path=ATOMIC)
    maxp, m = buf.max_particles, 5
    exp = yr.body_summary_ref(buf, yc.body_labels(buf), m)
    seen = []
    for mask in range(1, 8):
        # sentinels around the outputs: a guard word before and behind each
        mem = [torch.full((n + 4,), SENTINEL, dtype=dt, device="cuda") for n, dt in ((m * 24, torch.float32), (m * 8, torch.int64), (maxp, torch.int32))]
        out, counts, rank = ((x[2:-2] if mask & (1 << i) else False) for i, x in enumerate(mem))
        res = eng.body_summary(rows=m, out=out, counts=counts, rank=rank)
        res = res if isinstance(res, tuple) else (res,)
        assert len(res) == 1 + bool(mask & 2) + bool(mask & 4) and (res[0] is None) == (not mask & 1)
        got = tuple(x[2:-2].cpu().numpy().reshape(s) if mask & (1 << i) else None for i, (x, s) in enumerate(zip(mem, ((m, 24), (m, 8), (maxp,)))))
        yr.assert_equal(got, exp, "mask %d" % mask)
        for i, x in enumerate(mem):
            edge = x.cpu().numpy()
            assert (edge[:2] == SENTINEL).all() and (edge[-2:] == SENTINEL).all(), (mask, i)
            assert mask & (1 << i) or (edge == SENTINEL).all(), (mask, i)
        seen.append(tuple(None if g is None else g.tobytes() for g in got))
    again = call(eng, m)
    assert tuple(g.tobytes() for g in again) == seen[-1] == tuple(g.tobytes() for g in call(eng, m))     # identical bytes
    host = eng.body_summary_host(rows=m)
    assert tuple(g.tobytes() for g in host) == seen[-1] and host[1].dtype == np.int64
    lab = yc.caller_labels(buf, "stripes")
    yr.assert_equal(eng.body_summary_host(lab, rows=m), yr.body_summary_ref(buf, lab, m), "host variant, caller's labels")
    eng.destroy()


# 12
@pytest.mark.parametrize("what,mk,kw", READ_ONLY, ids=[r[0] for r in READ_ONLY])
def test_read_only(sb, what, mk, kw):
    """frame, body_summary, frame == frame, frame: the read-back byte for byte, the summary row, the promise flags and the schedule"""
    import torch

    def calls(eng, case):
        eng.body_summary(counts=True, rank=True)
        eng.body_summary(torch.from_numpy(yc.caller_labels(case["buf"], "stripes")).cuda(), rows=3)
        eng.body_summary_host()
    rh.read_only(sb, what, mk, kw, lambda sb, case, **k: engine(sb, case["buf"], bounds=case["bounds"], **k), calls)


# 13
def test_stream_ordering(sb):
    """frame(), body_summary() and a torch reduction on a side stream taken from a second Engine, no sync in between"""
    import torch
    case = sc.case_default(sb)
    buf = case["buf"]
    eng = engine(sb, buf, bounds=1000.0, collision_mode=GRID)
    other = engine(sb, buf, bounds=1000.0, collision_mode=GRID)
    side = torch.cuda.ExternalStream(other.stream(), device=torch.device("cuda", eng.device))
    with torch.cuda.stream(side):
        eng.frame()
        eng.frame()
        rows, counts, rank = eng.body_summary(rows=16, counts=True, rank=True)
        biggest = (rank == 0).sum()
        got = (rows.clone(), counts.clone(), rank.clone())
    side.synchronize()
    now = eng.load_buffers(buf.copy())
    yr.assert_equal(tuple(x.cpu().numpy() for x in got), yr.body_summary_ref(now, yc.body_labels(now), 16), "ordering")
    assert int(biggest) == int(got[1][0, 0])
    other.destroy()
    eng.destroy()


# 14
def test_info_keys(sb):
    buf = yc.scene(sb, "path 65 in 65/64")
    eng = engine(sb, buf, path=ATOMIC)
    assert eng.info("body_summary_kernel_scratch_bytes") == 0
    assert 0 < eng.info("body_summary_kernel_vgprs") <= 64
    assert eng.info("body_summary_table_build_us") == 0 and eng.info("body_summary_scratch_bytes") == 0
    eng.body_summary()
    assert eng.info("body_summary_table_build_us") > 0
    # W of 65 is 128: 137 bytes a position (the carving rounds 16 arrays up to 256 bytes each), the engine's own labels at 4 bytes
    # a particle of capacity, and the two tables: 4 bytes a data index, 16 bytes a caller beam slot
    assert 137 * 128 <= eng.info("body_summary_scratch_bytes") <= 137 * 128 + 16 * 256 + 4 * 65 + 4 * 65 + 16 * 64
    eng.destroy()


# 15
def test_errors_on_a_live_engine(sb):
    import torch
    buf = sc.case_default(sb)["buf"]
    eng = sb.Engine(bounds_size=1000.0, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=OFF)
    with pytest.raises(sb.EngineError) as e:
        eng.body_summary()
    assert e.value.status == 5          # SB_ERR_STATE
    with pytest.raises(sb.EngineError) as e:
        eng.body_summary_host()
    assert e.value.status == 5
    eng.write_buffers(buf)
    with pytest.raises(sb.EngineError) as e:
        eng.body_summary(out=False)
    assert e.value.status == 1          # SB_ERR_INVALID: three NULL outputs
    with pytest.raises(ValueError):
        eng.body_summary(rows=0)
    with pytest.raises(ValueError):
        eng.body_summary(rows=buf.max_particles + 1)
    mem = torch.empty(32 * buf.max_particles, dtype=torch.int32, device="cuda")
    for kw in (dict(out=mem.data_ptr() + 2), dict(rank=mem.data_ptr() + 1), dict(counts=mem.data_ptr() + 4), dict(labels=mem.data_ptr() + 2)):
        with pytest.raises(sb.EngineError) as e:
            eng.body_summary(**kw)
        assert e.value.status == 1, kw
    L, vp = sb.engine.load_library(), ctypes.c_void_p
    o = sb.engine.SbBodySummaryOptions()
    size = ctypes.sizeof(o)
    for struct_size, reserved, rows in ((size - 4, 0, 4), (size + 8, 0, 4), (size, 7, 4), (size, 0, 0), (size, 0, buf.max_particles + 1)):
        o.struct_size, o.reserved[4], o.max_rows = struct_size, reserved, rows
        assert L.sb_body_summary_device(eng._h, ctypes.byref(o), None, vp(mem.data_ptr()), None, None) == 1, (struct_size, reserved, rows)
        host = np.empty((8, 24), np.float32)
        assert L.sb_body_summary(eng._h, ctypes.byref(o), None, host.ctypes.data_as(vp), None, None) == 1, (struct_size, reserved, rows)
    o.struct_size, o.reserved[4], o.max_rows = size, 0, 4
    assert L.sb_body_summary_device(eng._h, ctypes.byref(o), None, vp(mem.data_ptr()), None, None) == 0   # ... and the engine still works
    assert L.sb_body_summary_device(eng._h, None, None, None, None, None) == 1
    eng.halo_configure([0, 1], [2, 3])
    with pytest.raises(sb.EngineError) as e:
        eng.body_summary()
    assert e.value.status == 6          # SB_ERR_UNSUPPORTED
    eng.destroy()


# 16
@needs_node
def test_node_body_summary_equals_pythons(sb):
    r = run_node("body_summary.gpu.test.js")
    assert r["ok"], r
    buf = sb.scenes.default_buffers(1, 128, 320)
    eng = sb.Engine(bounds_size=1000.0, particle_radius=10.0, subticks=64, layout=1, max_particles=128, max_beams=320,
                    collision_mode=OFF)
    eng.write_buffers(buf)
    eng.frame()
    rows, counts, rank = eng.body_summary_host(rows=12)
    now = eng.load_buffers(buf.copy())
    eng.destroy()
    yr.assert_equal((rows, counts, rank), yr.body_summary_ref(now, yc.body_labels(now), 12), "python against the reference")
    assert r["rowBits"] == rows.view(np.uint32).ravel().tolist()
    assert r["counts"] == [float(c) for c in counts.ravel()] and r["rank"] == rank.tolist() and counts[8, 0] == 1 and counts[9, 2] == -1
