"""BatchEngine.raycast (sb_batch_raycast_device) on the GPU, every comparison bit for bit (np.array_equal): t, hit
and counts equal tests/batch_raycast_ref.py on what load_scene returns -- the twelve scenes of the CPU case set in both collision
modes, without and with labels; after a cut and the frame that removes the cut beams; after add_particles and add_beams; after
reset and fork; with bodies()' labels and with stale arbitrary ones; the call only reads; each output alone; argument errors
enqueue nothing; the kernel uses no scratch.  Outputs are pre-filled with a pattern: an unwritten word would show."""
import ctypes

import numpy as np
import pytest

import batch_add_beams_cases as add_cases
import batch_raycast_cases as cases
import batch_raycast_ref as ref
from batch_harness import load_all
from batch_query_rig import GRID, OFF, batch, dev, query, raw
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

F = np.float32
INF = ref.INF

cast, check = query("raycast", ref.raycast_of, ref.RayCast, ref.same, (("t", (), "float32"), ("hit", (3,), "int32"), ("counts", None, "int32")))


def at_beams(buf, ds, off=4.0):
    """one BEAMS-only row per beam data index: across its middle from `off` away, tmax twice that"""
    rows = []
    for d in ds:
        pa, pb = (buf.particles[int(buf.beams[e][d]), :2].astype(np.float64) for e in ("a", "b"))
        mid, e = 0.5 * (pa + pb), (pb - pa) / np.hypot(*(pb - pa))
        n = np.array([-e[1], e[0]])
        rows.append((ref.BEAMS, *(mid + off * n + 1.5 * e), *(-n), 2.0 * off))
    return rows


@pytest.mark.parametrize("mode", [OFF, GRID])
def test_case_set(sb, mode):
    """1: the twelve scenes of the CPU case set, one of them never uploaded, without and with their labels"""
    cs = cases.case_set(sb)
    bufs, rows, labels = cases.stacked(cs)
    be = batch(sb, bufs, mode)
    for lab, key in ((None, "expect"), (labels, "expect_labelled")):
        _, got = check(be, bufs, rows, lab, "case set, labels %s" % (lab is not None))
        for i, c in enumerate(cs):
            for j, (t, kind, index) in c[key].items():
                assert (got.t[i, j].view(np.uint32), got.hit[i, j, 0], got.hit[i, j, 1]) == (F(t).view(np.uint32), kind, index), (c["name"], j)
        assert set(got.hit[9, :, 0].tolist()) <= {-2, 0, 3} and got.counts[9, 1:3].tolist() == [0, 0] and got.counts[9, 3] >= 5, "never uploaded: the walls are still there"
        assert set(got.hit[..., 0].ravel().tolist()) == {-2, -1, 0, 1, 2, 3}
    be.destroy()


def test_cut_then_frame(sb):
    """2: a cut beam still stops a ray while its flag is pending; after the frame whose delete pass removes it, it does not"""
    buf = sb.scenes.default_buffers(cases.LAYOUT, *cases.CAP)
    bufs = [buf, buf]
    be = batch(sb, bufs, GRID)
    first, second = [10, 150], [60, 220]
    shapes = np.stack([add_cases.quarter_discs(buf, first)] * 2)
    _, c = be.cut(dev(shapes))
    maxP = buf.max_particles
    cut_a = [int(buf.mapping[maxP + s]) for s in first]
    rows = np.stack([ref.pack(at_beams(buf, cut_a))] * 2)
    _, got = check(be, bufs, rows, None, "a cut pending")
    n_cut = c.cpu().numpy()[:, 1]
    assert (n_cut >= 2).all() and got.hit[0, :, :2].tolist() == [[2, d] for d in cut_a], "pending: still met"
    be.frame()
    now = load_all(be, bufs)
    assert now[0].beam_count == buf.beam_count - n_cut[0], "the frame removed the cut beams"
    cut_b = [int(now[0].mapping[maxP + s]) for s in second]
    be.cut(dev(np.stack([add_cases.quarter_discs(now[0], second)] * 2)))
    rows = np.stack([ref.pack(at_beams(now[0], cut_a + cut_b))] * 2)
    _, got = check(be, bufs, rows, None, "removed and pending")
    assert not set(got.hit[0, :2, 1].tolist()) & set(cut_a), "removed: no longer met"
    assert got.hit[0, 2:, :2].tolist() == [[2, d] for d in cut_b], "pending: still met"
    be.destroy()


def test_spawn_weld_reset_fork(sb):
    """3, 4: a spawned particle and a weld are met; reset() takes them away again; a forked scene answers as its source"""
    import torch
    buf = sb.scenes.default_buffers(cases.LAYOUT, *cases.CAP)
    bufs = [buf, buf]
    be = batch(sb, bufs)
    rows = np.stack([ref.pack([(7, 600, 700, 0, 1, INF), (ref.BEAMS, 625, 700, 0, 1, INF), (7, 625, 700, 0, 1, INF)])] * 2)
    _, before = check(be, bufs, rows, None, "uploaded")
    pos = torch.tensor([[[600.0, 800.0], [650.0, 800.0]], [[0.0, 0.0], [0.0, 0.0]]], device="cuda")
    valid = torch.tensor([[True, True], [False, False]], device="cuda")
    res, _ = be.add_particles(sb.batch.new_particle_rows(pos, valid=valid))
    new = res.cpu().numpy()
    assert (new[0] >= 119).all() and (new[1] < 0).all()
    wres, _ = be.add_beams(sb.batch.new_beam_rows(res.reshape(2, 1, 2).contiguous(), 50.0, 700.0, 0.2, 1.0e9), length_current=True)
    weld = wres.cpu().numpy()
    assert weld[0, 0] >= 299 and weld[1, 0] < 0
    _, got = check(be, bufs, rows, None, "spawned and welded")
    assert got.t[0].tolist() == [90.0, 100.0, 100.0] and got.hit[0, :, :2].tolist() == [[1, new[0, 0]], [2, weld[0, 0]], [2, weld[0, 0]]]
    assert ref.same(ref.RayCast(*(x[1] for x in got)), ref.RayCast(*(x[1] for x in before))) == [], "scene 1 as it was"
    be.fork(torch.tensor([0, 0], dtype=torch.int32, device="cuda"))
    _, forked = check(be, bufs, rows, None, "forked")
    assert all(np.array_equal(x[0], x[1]) for x in forked) and forked.hit[1, 0, 1] == new[0, 0]
    be.reset()
    _, again = check(be, bufs, rows, None, "reset")
    assert ref.same(again, before) == [] and (again.hit[:, 1, 0] == 0).all()
    be.destroy()


def test_labels(sb):
    """5, 6: labels=True == bodies()'s labels passed explicitly == the restatement with them; stale arbitrary labels are only
    compared: defined outputs, equal to the restatement with the same labels"""
    cs = cases.case_set(sb)
    bufs, rows, labels = cases.stacked(cs)
    be = batch(sb, bufs)
    lab, _ = be.bodies()
    assert np.array_equal(lab.cpu().numpy(), labels), "the host's labels of the case set are bodies()'s"
    a, b = cast(be, rows, True), cast(be, rows, labels)
    assert ref.same(a, b) == [] and ref.same(a, ref.raycast_of(load_all(be, bufs), rows, labels=labels)) == []
    rng = np.random.default_rng(9)
    stale = rng.integers(-2 ** 31, 2 ** 31, labels.shape, dtype=np.int64).astype(np.int32)
    stale[:, ::3] = rng.integers(0, 5, stale[:, ::3].shape)
    stale[:, 1::7] = np.array([2 ** 31 - 1, -2 ** 31, 10 ** 6, -5], np.int32)[rng.integers(0, 4, stale[:, 1::7].shape)]
    skipping = rows.copy()
    skipping[:, ::2, 6] = rng.integers(0, 5, skipping[:, ::2, 6].shape)
    skipping[:, 1, 6] = np.uint32(2 ** 31 - 1)
    _, got = check(be, bufs, skipping, stale, "stale labels")
    assert ref.same(got, ref.raycast_of(load_all(be, bufs), skipping, labels=labels)) != [], "the labels matter"
    be.destroy()


def test_read_only(sb):
    """7: no byte of state_tensors(), summary() and bodies() changes over a raycast(); frame, raycast, frame == frame, frame"""
    buf = sb.scenes.default_buffers(cases.LAYOUT, *cases.CAP)
    bufs = [buf, buf]
    rows = np.stack([cases.case_set(sb)[4]["rows"]] * 2)
    a, b = batch(sb, bufs, GRID), batch(sb, bufs, GRID)
    before = raw(a)
    cast(a, rows)
    cast(a, rows, True)
    assert raw(a) == before
    a.frame()
    b.frame()
    cast(a, rows)
    cast(a, rows, True)
    a.frame()
    b.frame()
    assert raw(a) == raw(b)
    for i, (x, y) in enumerate(zip(load_all(a, bufs), load_all(b, bufs))):
        assert_same(x, y, "scene %d: frame, raycast, frame == frame, frame" % i)
    a.destroy()
    b.destroy()


def test_each_output_alone(sb):
    """8: each output with the other two NULL; the defaults; k == 0"""
    import torch
    cs = cases.case_set(sb)
    bufs, rows, labels = cases.stacked(cs)
    be = batch(sb, bufs)
    full = cast(be, rows, labels)
    r, lab = dev(rows), dev(labels)
    for i, name in enumerate(ref.RayCast._fields):
        want = [False] * 3
        want[i] = True
        got = be.raycast(r, labels=lab, t=want[0], hit=want[1], counts=want[2])
        assert [x is not None for x in got] == want and np.array_equal(got[i].cpu().numpy().view(np.int32), full[i].view(np.int32)), name
    d = be.raycast(r, labels=lab)
    assert ref.same(ref.RayCast(*(x.cpu().numpy() for x in d)), full) == []
    z = be.raycast(r[:, :0].contiguous())
    assert z.t.shape == (12, 0) and z.hit.shape == (12, 0, 3) and not z.counts.cpu().numpy().any()
    packed = sb.batch.ray_rows(torch.tensor(rows[:, :, 1:3].copy().view(F)).cuda(), torch.tensor(rows[:, :, 3:5].copy().view(F)).cuda(),
                               torch.tensor(rows[:, :, 5].copy().view(F)).cuda(), mask=dev(rows[:, :, 0].copy()), skip_label=dev(rows[:, :, 6].copy()))
    assert np.array_equal(packed.cpu().numpy().view(np.uint32)[:, :, :7], rows[:, :, :7]) and not packed[:, :, 7].any(), "ray_rows packs the rows"
    be.destroy()


def test_errors_enqueue_nothing(sb):
    """9: a NULL handle, a flag bit, k above the limit, NULL rows, all outputs NULL, a misaligned pointer: SB_ERR_INVALID, and no
    output is touched; k == 0 is SB_OK and enqueues nothing"""
    import torch
    buf = sb.scenes.default_buffers(cases.LAYOUT, *cases.CAP)
    be = batch(sb, [buf])
    lib = sb.batch.load_library()
    vp = ctypes.c_void_p
    rows = dev(ref.pack([(ref.WALLS, 0, 50, 1, 0, INF)] * 257)[None])
    outs = [torch.full((n,), 77, dtype=torch.int32, device="cuda") for n in (257, 257 * 3, 4, 128)]
    r, (t, h, c, lab) = rows.data_ptr(), (x.data_ptr() for x in outs)
    be.sync()
    torch.cuda.synchronize()
    for hnd, flags, rp, k, args in ((None, 0, r, 4, (lab, t, h, c)), (be._h, 1, r, 4, (lab, t, h, c)), (be._h, 0x80000000, r, 4, (None, t, h, c)),
                                    (be._h, 0, r, 257, (lab, t, h, c)), (be._h, 0, None, 4, (lab, t, h, c)), (be._h, 0, r, 4, (lab, None, None, None)),
                                    (be._h, 0, r, 0, (None, None, None, None)), (be._h, 0, r + 2, 4, (lab, t, h, c)), (be._h, 0, r, 4, (lab + 1, t, h, c)),
                                    (be._h, 0, r, 4, (lab, t + 2, h, c)), (be._h, 0, r, 4, (lab, t, h + 3, c)), (be._h, 0, r, 4, (lab, t, h, c + 2))):
        assert lib.sb_batch_raycast_device(hnd, flags, vp(rp), k, *[vp(p) for p in args]) == 1, (flags, k, args)
    assert b"aligned" in lib.sb_batch_last_error(be._h)
    assert lib.sb_batch_raycast_device(be._h, 0, None, 0, None, vp(t), vp(h), vp(c)) == 0, "no rays: nothing done"
    be.sync()
    assert all((x.cpu().numpy() == 77).all() for x in outs), "no output was touched"
    for bad in (rows[:, :, :7].contiguous(), torch.zeros((2, 4, 8), dtype=torch.int32, device="cuda"), rows, rows[:, :4].to(torch.int64)):
        with pytest.raises(ValueError):
            be.raycast(bad)
    with pytest.raises(ValueError):
        be.raycast(rows[:, :4].contiguous(), t=False, hit=False, counts=False)
    with pytest.raises(ValueError):
        be.raycast(rows[:, :4].contiguous(), t=torch.zeros(3, dtype=torch.float32, device="cuda"))
    assert lib.sb_batch_raycast_device(be._h, 0, vp(r), 4, None, vp(t), vp(h), vp(c)) == 0
    be.sync()
    assert outs[2].cpu().numpy().tolist() == [4, 0, 0, 4] and outs[0].cpu().numpy()[:5].view(F).tolist()[:4] == [1000.0] * 4 and outs[0][4] == 77
    be.destroy()


def test_kernel_resources(sb):
    """10: no scratch; the info keys"""
    be = sb.BatchEngine(n_scenes=1, max_particles=1024, max_beams=4096)
    assert be.info("raycast_kernel_scratch_bytes") == 0 and 0 < be.info("raycast_kernel_vgprs") <= 128
    assert (be.info("ray_max"), be.info("ray_hit_words"), be.info("ray_count_words")) == (256, 3, 4)
    assert be.info("raycast_lds_bytes") == (2 * 256 + 4 * 1024 + 4096 + 8 * 256 + 4) * 4 <= 65536
    be.destroy()
