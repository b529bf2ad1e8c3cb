"""BatchEngine.nearest (sb_batch_nearest_device) on the GPU, every comparison bit for bit (np.array_equal): d, hit,
point, within and counts equal tests/batch_nearest_ref.py on what load_scene returns -- the twelve scenes of the CPU case set in both
collision modes, without and with labels; after a frame; after a cut and the frame that removes the cut beams; after add_particles
and add_beams; after reset and fork; with bodies()' labels and with stale arbitrary ones; the call only reads; each output alone;
argument errors enqueue nothing; the kernel uses no scratch; the grasp recipe end to end.  Outputs are pre-filled with a pattern:
an unwritten word would show."""
import ctypes

import numpy as np
import pytest

import batch_add_beams_cases as add_cases
import batch_add_beams_ref as add_ref
import batch_nearest_cases as cases
import batch_nearest_ref as ref
from batch_harness import load_all
from batch_query_rig import GRID, OFF, batch, dev, query, raw
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

F = np.float32
INF = ref.INF

ask, check = query("nearest", ref.nearest_of, ref.Nearest, ref.same, (("d", (), "float32"), ("hit", (3,), "int32"), ("point", (2,), "float32"),
                                                                      ("within", (2,), "int32"), ("counts", None, "int32")))


def on_beams(buf, ds):
    """one BEAMS-only row per beam data index: a quarter along it (no other beam of the default scene passes there), reach 2"""
    rows = []
    for d in ds:
        pa, pb = (buf.particles[int(buf.beams[e][d]), :2].astype(np.float64) for e in ("a", "b"))
        rows.append((ref.BEAMS, *(0.75 * pa + 0.25 * pb), 2.0))
    return rows


@pytest.mark.parametrize("mode", [OFF, GRID])
def test_case_set(sb, mode):
    """1: the twelve scenes of the CPU case set, one of them never uploaded, without and with their labels; then after a frame"""
    cs = cases.case_set(sb)
    bufs, rows, labels = cases.stacked(cs)
    be = batch(sb, bufs, mode)
    never = cases.NEVER_UPLOADED
    for lab, key, wkey in ((None, "expect", None), (labels, "expect_labelled", "expect_within_labelled")):
        _, got = check(be, bufs, rows, lab, "case set, labels %s" % (lab is not None))
        for i, c in enumerate(cs):
            for j, (d, kind, index, qx, qy) in c[key].items():
                have = (got.d[i, j].view(np.uint32), got.hit[i, j, 0], got.hit[i, j, 1], *got.point[i, j].view(np.uint32))
                assert have == (F(d).view(np.uint32), kind, index, F(qx).view(np.uint32), F(qy).view(np.uint32)), (c["name"], j, have)
            for j, want in {**c["expect_within"], **(c[wkey] if wkey else {})}.items():
                if got.hit[i, j, 0] >= 0:
                    assert tuple(got.within[i, j]) == want, (c["name"], j)
        assert set(got.hit[never, :, 0].tolist()) <= {-2, -1, 0, 3} and not got.within[never].any() and got.counts[never, 1:3].tolist() == [0, 0], "never uploaded: walls only"
        assert got.counts[never, 3] >= 1
        assert set(got.hit[..., 0].ravel().tolist()) == {-2, -1, 0, 1, 2, 3}
    be.frame()
    check(be, bufs, rows, labels, "after a frame")
    be.destroy()


def test_cut_then_frame(sb):
    """2: a cut beam is still near while its flag is pending; after the frame whose delete pass removes it, it is not"""
    buf = sb.scenes.default_buffers(cases.LAYOUT, *cases.CAP)
    bufs = [buf, buf]
    be = batch(sb, bufs, GRID)
    first, second = [10, 150], [60, 220]
    shapes = np.stack([add_cases.quarter_discs(buf, first)] * 2)
    _, c = be.cut(dev(shapes))
    maxP = buf.max_particles
    cut_a = [int(buf.mapping[maxP + s]) for s in first]
    rows = np.stack([ref.pack(on_beams(buf, cut_a))] * 2)
    _, got = check(be, bufs, rows, None, "a cut pending")
    n_cut = c.cpu().numpy()[:, 1]
    assert (n_cut >= 2).all() and got.hit[0, :, :2].tolist() == [[2, d] for d in cut_a], "pending: still there"
    be.frame()
    now = load_all(be, bufs)
    assert now[0].beam_count == buf.beam_count - n_cut[0], "the frame removed the cut beams"
    cut_b = [int(now[0].mapping[maxP + s]) for s in second]
    be.cut(dev(np.stack([add_cases.quarter_discs(now[0], second)] * 2)))
    rows = np.stack([ref.pack(on_beams(now[0], cut_a + cut_b))] * 2)
    _, got = check(be, bufs, rows, None, "removed and pending")
    assert not set(got.hit[0, :2, 1].tolist()) & set(cut_a), "removed: no longer there"
    assert got.hit[0, 2:, :2].tolist() == [[2, d] for d in cut_b], "pending: still there"
    be.destroy()


def test_spawn_weld_reset_fork(sb):
    """3: a spawned particle and a weld are found; reset() takes them away again; a forked scene answers as its source"""
    import torch
    buf = sb.scenes.default_buffers(cases.LAYOUT, *cases.CAP)
    bufs = [buf, buf]
    be = batch(sb, bufs)
    rows = np.stack([ref.pack([(7, 600, 790, 30), (ref.BEAMS, 625, 790, 30), (7, 625, 790, 30)])] * 2)
    _, before = check(be, bufs, rows, None, "uploaded")
    assert (before.hit[:, :, 0] == 0).all(), "nothing there yet"
    pos = torch.tensor([[[600.0, 800.0], [650.0, 800.0]], [[0.0, 0.0], [0.0, 0.0]]], device="cuda")
    valid = torch.tensor([[True, True], [False, False]], device="cuda")
    res, _ = be.add_particles(sb.batch.new_particle_rows(pos, valid=valid))
    new = res.cpu().numpy()
    assert (new[0] >= 119).all() and (new[1] < 0).all()
    wres, _ = be.add_beams(sb.batch.new_beam_rows(res.reshape(2, 1, 2).contiguous(), 50.0, 700.0, 0.2, 1.0e9), length_current=True)
    weld = wres.cpu().numpy()
    assert weld[0, 0] >= 299 and weld[1, 0] < 0
    _, got = check(be, bufs, rows, None, "spawned and welded")
    assert got.d[0].tolist() == [10.0, 10.0, 10.0] and got.hit[0, :, :2].tolist() == [[1, new[0, 0]], [2, weld[0, 0]], [2, weld[0, 0]]]
    assert got.point[0].tolist() == [[600.0, 800.0], [625.0, 800.0], [625.0, 800.0]] and got.within[0].tolist() == [[1, 1], [0, 1], [2, 1]]
    assert ref.same(ref.Nearest(*(x[1] for x in got)), ref.Nearest(*(x[1] for x in before))) == [], "scene 1 as it was"
    be.fork(torch.tensor([0, 0], dtype=torch.int32, device="cuda"))
    _, forked = check(be, bufs, rows, None, "forked")
    assert all(np.array_equal(x[0], x[1]) for x in forked) and forked.hit[1, 0, 1] == new[0, 0]
    be.reset()
    _, again = check(be, bufs, rows, None, "reset")
    assert ref.same(again, before) == []
    be.destroy()


def test_labels(sb):
    """4: labels=True == bodies()'s labels passed explicitly == the restatement with them; stale arbitrary labels are only
    compared: defined outputs, equal to the restatement with the same labels"""
    cs = cases.case_set(sb)
    bufs, rows, labels = cases.stacked(cs)
    be = batch(sb, bufs)
    lab, _ = be.bodies()
    assert np.array_equal(lab.cpu().numpy(), labels), "the host's labels of the case set are bodies()'s"
    a, b = ask(be, rows, True), ask(be, rows, labels)
    assert ref.same(a, b) == [] and ref.same(a, ref.nearest_of(load_all(be, bufs), rows, labels=labels)) == []
    rng = np.random.default_rng(9)
    stale = rng.integers(-2 ** 31, 2 ** 31, labels.shape, dtype=np.int64).astype(np.int32)
    stale[:, ::3] = rng.integers(0, 5, stale[:, ::3].shape)
    stale[:, 1::7] = np.array([2 ** 31 - 1, -2 ** 31, 10 ** 6, -5], np.int32)[rng.integers(0, 4, stale[:, 1::7].shape)]
    skipping = rows.copy()
    skipping[:, ::2, 4] = rng.integers(0, 5, skipping[:, ::2, 4].shape)
    skipping[:, 1, 4] = np.uint32(2 ** 31 - 1)
    _, got = check(be, bufs, skipping, stale, "stale labels")
    assert ref.same(got, ref.nearest_of(load_all(be, bufs), skipping, labels=labels)) != [], "the labels matter"
    be.destroy()


def test_read_only(sb):
    """5: no byte of state_tensors(), summary() and bodies() changes over a nearest(); frame, nearest, frame == frame, frame, on
    every report and on the exported state"""
    buf = sb.scenes.default_buffers(cases.LAYOUT, *cases.CAP)
    bufs = [buf, buf]
    rows = np.stack([cases.case_set(sb)[5]["rows"]] * 2)
    a, b = batch(sb, bufs, GRID), batch(sb, bufs, GRID)
    before = raw(a)
    ask(a, rows)
    ask(a, rows, True)
    assert raw(a) == before
    a.frame()
    b.frame()
    ask(a, rows)
    ask(a, rows, True)
    a.frame()
    b.frame()
    assert raw(a) == raw(b)
    for i, (x, y) in enumerate(zip(load_all(a, bufs), load_all(b, bufs))):
        assert_same(x, y, "scene %d: frame, nearest, frame == frame, frame" % i)
    a.destroy()
    b.destroy()


def test_each_output_alone(sb):
    """6: each output with the other four NULL; the defaults; k == 0; point_rows packs the rows"""
    import torch
    cs = cases.case_set(sb)
    bufs, rows, labels = cases.stacked(cs)
    be = batch(sb, bufs)
    full = ask(be, rows, labels)
    r, lab = dev(rows), dev(labels)
    for i, name in enumerate(ref.Nearest._fields):
        want = [False] * 5
        want[i] = True
        got = be.nearest(r, labels=lab, d=want[0], hit=want[1], point=want[2], within=want[3], counts=want[4])
        assert [x is not None for x in got] == want and np.array_equal(got[i].cpu().numpy().view(np.int32), full[i].view(np.int32)), name
    d = be.nearest(r, labels=lab)
    assert all(x is not None for x in d) and ref.same(ref.Nearest(*(x.cpu().numpy() for x in d)), full) == []
    z = be.nearest(r[:, :0].contiguous())
    assert z.d.shape == (12, 0) and z.hit.shape == (12, 0, 3) and z.point.shape == (12, 0, 2) and not z.counts.cpu().numpy().any()
    packed = sb.batch.point_rows(torch.tensor(rows[:, :, 1:3].copy().view(F)).cuda(), torch.tensor(rows[:, :, 3].copy().view(F)).cuda(),
                                 mask=dev(rows[:, :, 0].copy()), skip_label=dev(rows[:, :, 4].copy()))
    assert np.array_equal(packed.cpu().numpy().view(np.uint32)[:, :, :5], rows[:, :, :5]) and not packed[:, :, 5:].any(), "point_rows packs the rows"
    be.destroy()


def test_errors_enqueue_nothing(sb):
    """7: a NULL handle, a flag bit, k above the limit, NULL rows, all outputs NULL, a misaligned pointer: SB_ERR_INVALID, and no
    output is touched; k == 0 is SB_OK and enqueues nothing"""
    import torch
    buf = sb.scenes.default_buffers(cases.LAYOUT, *cases.CAP)
    be = batch(sb, [buf])
    lib = sb.batch.load_library()
    vp = ctypes.c_void_p
    rows = dev(ref.pack([(ref.WALLS, 30, 50, INF)] * 257)[None])
    outs = [torch.full((n,), 77, dtype=torch.int32, device="cuda") for n in (257, 257 * 3, 257 * 2, 257 * 2, 4, 128)]
    r, (d, h, q, w, c, lab) = rows.data_ptr(), (x.data_ptr() for x in outs)
    be.sync()
    torch.cuda.synchronize()
    good = (lab, d, h, q, w, c)
    calls = [(None, 0, r, 4, good), (be._h, 1, r, 4, good), (be._h, 0x80000000, r, 4, (None,) + good[1:]), (be._h, 0, r, 257, good),
             (be._h, 0, None, 4, good), (be._h, 0, r, 4, (lab, None, None, None, None, None)), (be._h, 0, r, 0, (None,) * 6), (be._h, 0, r + 2, 4, good)]
    for i in range(6):      # each pointer in turn misaligned
        calls.append((be._h, 0, r, 4, tuple(p + (1 + i % 3) if j == i else p for j, p in enumerate(good))))
    for hnd, flags, rp, k, args in calls:
        assert lib.sb_batch_nearest_device(hnd, flags, vp(rp), k, *[vp(p) for p in args]) == 1, (flags, k, args)
    assert b"aligned" in lib.sb_batch_last_error(be._h)
    assert lib.sb_batch_nearest_device(be._h, 0, None, 0, None, vp(d), vp(h), vp(q), vp(w), vp(c)) == 0, "no points: nothing done"
    be.sync()
    assert all((x.cpu().numpy() == 77).all() for x in outs), "no output was touched"
    for bad in (rows[:, :, :7].contiguous(), torch.zeros((2, 4, 8), dtype=torch.int32, device="cuda"), rows, rows[:, :4].to(torch.int64)):
        with pytest.raises(ValueError):
            be.nearest(bad)
    with pytest.raises(ValueError):
        be.nearest(rows[:, :4].contiguous(), d=False, hit=False, point=False, within=False, counts=False)
    with pytest.raises(ValueError):
        be.nearest(rows[:, :4].contiguous(), d=torch.zeros(3, dtype=torch.float32, device="cuda"))
    assert lib.sb_batch_nearest_device(be._h, 0, vp(r), 4, None, vp(d), vp(h), vp(q), vp(w), vp(c)) == 0
    be.sync()
    assert outs[4].cpu().numpy().tolist() == [4, 0, 0, 4] and outs[0].cpu().numpy()[:5].view(F).tolist()[:4] == [30.0] * 4 and outs[0][4] == 77
    assert outs[2].cpu().numpy()[:9].view(F).tolist()[:8] == [0.0, 50.0] * 4 and outs[2][8] == 77 and not outs[3].cpu().numpy()[:8].any() and outs[3][8] == 77
    be.destroy()


def test_kernel_resources(sb):
    """8: no scratch; the info keys; three workgroups' LDS fit a CU's 160 KiB at full capacity"""
    be = sb.BatchEngine(n_scenes=1, max_particles=1024, max_beams=4096)
    assert be.info("nearest_kernel_scratch_bytes") == 0 and 0 < be.info("nearest_kernel_vgprs") <= 128
    assert (be.info("near_max"), be.info("near_hit_words"), be.info("near_count_words")) == (256, 3, 4)
    assert be.info("nearest_lds_bytes") == (2 * 256 + 4 * 1024 + 4096 + 8 * 256 + 2 * 256 + 4) * 4 and 3 * be.info("nearest_lds_bytes") <= 160 * 1024
    be.destroy()


def test_grasp_recipe(sb):
    """9: the docstring's recipe end to end -- nearest() finds each hand's partner, add_beams() welds it, nothing is read back in
    between -- against the restatement followed by the add-beams restatement"""
    import torch
    b = sb.batch
    buf = sb.scenes.default_buffers(cases.LAYOUT, *cases.CAP)
    bufs = [buf, buf, buf]
    be = batch(sb, bufs)
    hands = np.array([[44], [45], [0]], np.int32)           # data indices of each scene's hand particle
    reach = np.array([[40.0], [1.0], [95.0]], F)              # scene 1: nothing within reach
    lab, _ = be.bodies()
    p, _, _ = be.state_tensors()
    hand = torch.from_numpy(hands).cuda()
    hand_pos = torch.gather(p[:, :, :2], 1, hand.long()[:, :, None].expand(-1, -1, 2)).contiguous()
    hand_label = torch.gather(lab, 1, hand.long())
    rows = b.point_rows(hand_pos, torch.from_numpy(reach).cuda(), mask=b.NEAR_PARTICLES, skip_label=hand_label)
    near = be.nearest(rows, labels=lab)
    partner = torch.where(near.hit[..., 0] == b.NEAR_PARTICLE, near.hit[..., 1], -1)
    pairs = torch.stack((partner, hand.expand_as(partner)), -1)
    result, counts = be.add_beams(b.new_beam_rows(pairs, 50.0, 700.0, 0.2, 1.0e9), length_current=True, skip_joined=True)
    # the same on the host
    labels = np.stack([ref.bodies_labels(buf)] * 3)
    want = ref.nearest_of(bufs, rows.cpu().numpy().view(np.uint32), labels=labels)
    assert ref.same(ref.Nearest(*(x.cpu().numpy() for x in near)), want) == []
    want_partner = np.where(want.hit[..., 0] == ref.PARTICLE, want.hit[..., 1], -1)
    assert want_partner[0, 0] >= 0 and want_partner[1, 0] == -1 and want_partner[2, 0] >= 0, want_partner
    assert (labels[[0, 2], want_partner[[0, 2], 0]] != labels[[0, 2], hands[[0, 2], 0]]).all(), "the partner is of another body"
    now = load_all(be, bufs)
    for i in range(3):
        beam_rows = add_ref.pack([(int(want_partner[i, 0]), int(hands[i, 0]), 0.0, 50.0, 700.0, 0.2, 1.0e9)])
        exp, res, cnt = add_ref.add_ref(buf, beam_rows, add_ref.LENGTH_CURRENT | add_ref.SKIP_JOINED, add_ref.alive_set(buf))
        assert result.cpu().numpy()[i].tolist() == res.tolist() and counts.cpu().numpy()[i].tolist() == cnt, i
        assert_same(now[i], exp, "scene %d: the weld" % i)
    assert result.cpu().numpy()[:, 0].tolist() == [299, add_ref.EMPTY, 299]
    be.destroy()
