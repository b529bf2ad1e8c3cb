"""BatchEngine.graph (sb_batch_graph_device) on the GPU, every comparison bit for bit (np.array_equal): the five
outputs equal tests/graph_ref.py on what load_scene returns -- after cuts, welds and frames in which beams break; at the capacity
corners; under a sparse, permuted mapping; with and without SKIP_PENDING; around add_beams, reset, checkpoint and fork; the call
only reads; it agrees with bodies() and summary(); argument errors enqueue nothing; the kernel uses no scratch."""
import ctypes

import numpy as np
import pytest

import batch_add_beams_cases as add_cases
import cut_cases
import graph_cases
import graph_ref as ref
from batch_harness import load_all, make_batch, upload_each
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

OFF, GRID = 0, 2


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def batch(sb, case, mode=OFF):
    be = make_batch(sb, dict(case, mode=mode), mode=mode)
    upload_each(be, case["bufs"])
    return be


def graph(be, **kw):
    """all five outputs as numpy, written into tensors the test filled with a pattern first: every word is written"""
    import torch
    n, maxp, maxb = be.n_scenes, be.max_particles, be.max_beams
    fill = lambda shape, dt: torch.full(shape, -1515870811 if dt == torch.int32 else -7.25, dtype=dt, device="cuda")   # 0xA5A5A5A5
    g = be.graph(ends=fill((n, maxb, 2), torch.int32), material=fill((n, maxb, 5), torch.float32),
                 adjacency=(fill((n, maxp + 1), torch.int32), fill((n, 2 * maxb, 2), torch.int32)), counts=fill((n, 4), torch.int32), **kw)
    return ref.Graph(*(x.cpu().numpy() for x in g))


def check(be, bufs, what):
    """graph() == the restatement on what load_scene returns now; returns (scenes as read back, the graph)"""
    now = load_all(be, bufs)
    want = ref.graph_of(now, be.max_particles, be.max_beams)
    got = graph(be)
    print(what, "counts", got.counts.tolist(), "want", want.counts.tolist())
    assert ref.same(got, want) == [], what
    return now, got


def raw(be):
    """every byte the other reports can see: state rows, summary, bodies"""
    p, b, a = be.state_tensors()
    return [x.cpu().numpy().tobytes() for x in (p, b, a, be.summary(), *be.bodies())]


def default_shapes(case):
    """each of the case's default scenes cut by its own shapes: the strokes and discs of cut_cases over a box that moves with the scene"""
    names = ["vertical stroke", "horizontal stroke", "diagonal stroke", "disc", "stroke, none, disc"]
    shapes = np.zeros((len(case["bufs"]), 3, 8), np.uint32)
    for i, b in enumerate(case["bufs"]):
        x0, y0, x1, y1 = cut_cases.box_of(b)
        if i >= len(names):   # (the second round of the names: over the right half of the scene, a little lower)
            x0, y1 = (x0 + x1) / 2, y1 - 100.0
        sh = cut_cases.scene_shapes((x0 + 9.0 * i, y0, x1 - 5.0 * i, y1 + 3.0 * i))[names[i % len(names)]]
        shapes[i, :len(sh)] = sh
    return shapes


def cut_and_weld(sb, mode=OFF):
    case = add_cases.default_case(sb)
    be = batch(sb, case, mode)
    _, c = be.cut(dev(default_shapes(case)))
    _, a = be.add_beams(dev(case["rows"]))
    return case, be, c.cpu().numpy(), a.cpu().numpy()


def test_cut_welded_and_stepped_scenes(sb):
    """1: eight default scenes, each cut and welded differently; then two frames, in which the cut beams are removed and scene 2's
    brittle weld breaks"""
    case, be, c, a = cut_and_weld(sb, GRID)
    assert (c[:, 1] > 0).all() and a[:, 0].min() >= 5
    before, g0 = check(be, case["bufs"], "cut and welded")
    assert g0.counts[:, 0].tolist() == [299 + int(x) for x in a[:, 0]], "a pending cut is still listed, a weld is"
    be.frame(2)
    after, g1 = check(be, case["bufs"], "two frames later")
    assert all(y.beam_count <= x.beam_count - int(h) for x, y, h in zip(before, after, c[:, 1]))
    assert after[2].beam_count < before[2].beam_count - int(c[2, 1]), "the brittle weld broke too"
    assert ref.same(g0, g1) != []
    be.destroy()


def test_capacity_corners(sb):
    """2: a star of degree 4096 at full capacity, 2 particles / 1 beam, no beam, never uploaded, a chain of 65"""
    bufs = graph_cases.corner_scenes(sb)
    be = batch(sb, dict(layout=2, cap=graph_cases.CORNER_CAP, bufs=bufs))
    _, g = check(be, bufs, "corners")
    assert g.counts.tolist() == [[4096, 1024, 4096, 0], [1, 2, 1, 0], [0, 0, 0, -1], [0, 0, 0, -1], [64, 65, 2, 1]]
    assert (g.ends[3] == -1).all() and (g.nbr[3] == -1).all() and not g.row_ptr[3].any() and not g.material[3].view(np.uint32).any()
    # parts of the outputs: the default is ends and counts; counts alone; row_ptr without nbr
    d = be.graph()
    assert d.material is None and d.row_ptr is None and d.nbr is None
    assert np.array_equal(d.ends.cpu().numpy(), g.ends) and np.array_equal(d.counts.cpu().numpy(), g.counts)
    o = be.graph(ends=False, counts=True)
    assert o.ends is None and np.array_equal(o.counts.cpu().numpy(), g.counts)
    r = be.graph(ends=False, adjacency=(True, False), counts=False)
    assert r.nbr is None and r.counts is None and np.array_equal(r.row_ptr.cpu().numpy(), g.row_ptr)
    m = be.graph(ends=False, material=True, counts=False)
    assert np.array_equal(m.material.cpu().numpy().view(np.uint32), g.material.view(np.uint32))
    be.destroy()


def test_sparse_permuted_mapping(sb):
    """3: particle slot s at data index (5 s + 2) mod 32, beam slot s at (7 s + 3) mod 64: slots and data indices differ, with gaps"""
    case = add_cases.sparse_case(sb)
    be = batch(sb, case)
    now, g = check(be, case["bufs"], "sparse")
    buf = case["bufs"][0]
    slots = np.arange(30)
    d = buf.mapping[32:62].astype(np.int64)
    assert not np.array_equal(d, slots) and np.array_equal(g.ends[0, d, 0], buf.beams["a"][d]) and (g.ends[0, np.setdiff1d(np.arange(64), d)] == -1).all()
    assert g.counts[0].tolist() == [30, 14, 8, 0]
    be.destroy()


def test_pending_flags(sb):
    """4: after a cut, graph(skip_pending=True) == graph() after the delete pass; graph() before the pass still lists the cut beams"""
    case = add_cases.default_case(sb)
    be = batch(sb, case)
    hit, c = be.cut(dev(default_shapes(case)), hit=True)
    hit, c = hit.cpu().numpy().astype(bool), c.cpu().numpy()
    now, g_all = check(be, case["bufs"], "a cut pending")
    g_skip = graph(be, skip_pending=True)
    assert hit.sum() == c[:, 1].sum() > 0 and (g_all.ends[hit] >= 0).all() and (g_skip.ends[hit] == -1).all()
    assert g_all.counts[:, 0].tolist() == [299] * 8 and g_skip.counts[:, 0].tolist() == (299 - c[:, 1]).tolist()
    want = ref.graph_of(now, be.max_particles, be.max_beams, drop=[np.flatnonzero(h) for h in hit])
    assert ref.same(g_skip, want) == [], "skip_pending == the restatement without the hit beams"
    be.delete_pass()
    _, g_after = check(be, case["bufs"], "after the delete pass")
    assert ref.same(g_skip, g_after) == [], "skip_pending is what the delete pass leaves"
    assert ref.same(graph(be, skip_pending=True), g_after) == []
    be.destroy()


def test_lifecycle(sb):
    """5: add_beams, reset, checkpoint and fork around a graph"""
    import torch
    case = add_cases.sparse_case(sb)
    buf, rows = case["bufs"][0], case["rows"]
    be = batch(sb, case)
    _, g_up = check(be, case["bufs"], "uploaded")
    res, _ = be.add_beams(dev(rows))
    welded = res.cpu().numpy()[0]
    assert welded.tolist() == [4, 5, 6, 11, 12] and (g_up.ends[0, welded] == -1).all()
    _, g_add = check(be, case["bufs"], "welded")
    assert g_add.ends[0, welded].tolist() == [[int(r[0]), int(r[1])] for r in rows[0].view(np.int32)[:, :2]]
    assert g_add.material[0, welded].view(np.uint32).tolist() == rows[0][:, 2:7].view(np.uint32).tolist(), "the rows' materials, verbatim"
    be.reset()
    _, g_reset = check(be, case["bufs"], "reset")
    assert (g_reset.ends[0, welded] == -1).all() and ref.same(g_reset, g_up) == []
    be.add_beams(dev(rows))
    be.checkpoint()
    be.frame()
    be.reset()
    _, g_kept = check(be, case["bufs"], "welded, checkpoint, frame, reset")
    assert ref.same(g_kept, g_add) == []
    be.destroy()
    two = dict(case, bufs=[buf, buf], rows=np.stack([rows[0], np.full_like(rows[0], -1)]))
    be = batch(sb, two)
    be.add_beams(dev(two["rows"]))
    _, g = check(be, two["bufs"], "one of two welded")
    assert g.counts[:, 0].tolist() == [35, 30]
    be.fork(torch.tensor([0, 0], dtype=torch.int32, device="cuda"))
    _, g = check(be, two["bufs"], "forked")
    assert all(np.array_equal(x[0], x[1]) for x in (g.ends, g.material.view(np.uint32), g.row_ptr, g.nbr, g.counts)) and g.counts[1, 0] == 35
    be.destroy()


def test_read_only(sb):
    """6: no byte of state_tensors(), summary() and bodies() changes over a graph(); frame, graph, frame == frame, frame"""
    case, a, _, _ = cut_and_weld(sb, GRID)
    _, b, _, _ = cut_and_weld(sb, GRID)
    before = raw(a)
    graph(a)
    graph(a, skip_pending=True)
    assert raw(a) == before
    a.frame()
    b.frame()
    graph(a)
    graph(a, skip_pending=True)
    a.frame()
    b.frame()
    assert raw(a) == raw(b)
    for i, (x, y) in enumerate(zip(load_all(a, case["bufs"]), load_all(b, case["bufs"]))):
        assert_same(x, y, "scene %d: frame, graph, frame == frame, frame" % i)
    a.destroy()
    b.destroy()


def test_agrees_with_bodies_and_summary(sb):
    """7: both ends of a listed edge carry one label; listed edges per body == bodies(sizes=True)'s live beams; counts[:, 0] ==
    summary()[:, 1] -- with a cut pending, and after the frames that tear the bodies"""
    case, be, _, _ = cut_and_weld(sb)
    n_bodies = []
    for what in ("pending", "torn"):
        labels, counts, sizes = (x.cpu().numpy() for x in be.bodies(sizes=True))
        g = graph(be)
        assert np.array_equal(g.counts[:, 0], be.summary().cpu().numpy()[:, 1].astype(np.int32)), what
        for s in range(be.n_scenes):
            listed = g.ends[s][g.ends[s, :, 0] >= 0]
            la, lb = labels[s][listed[:, 0]], labels[s][listed[:, 1]]
            assert np.array_equal(la, lb) and (la >= 0).all(), (what, s)
            assert np.array_equal(np.bincount(la, minlength=be.max_particles).astype(np.int32), sizes[s, :, 1]), (what, s)
        n_bodies.append(counts[:, 0].copy())
        be.frame(2)
    assert (n_bodies[1] > n_bodies[0]).any(), "the cuts tore bodies apart"
    be.destroy()


def test_errors_enqueue_nothing(sb):
    """8: a NULL handle, unknown flag bits, a misaligned pointer, nbr without row_ptr: SB_ERR_INVALID, and no output is touched"""
    import torch
    case = add_cases.sparse_case(sb)
    be = batch(sb, case)
    lib = sb.batch.load_library()
    vp = ctypes.c_void_p
    outs = [torch.full((n,), 77, dtype=torch.int32, device="cuda") for n in (64 * 2, 64 * 5, 33, 128 * 2, 4)]
    e, m, r, nb, c = (x.data_ptr() for x in outs)
    be.sync()
    torch.cuda.synchronize()
    for h, flags, args in ((None, 0, (e, m, r, nb, c)), (be._h, 2, (e, m, r, nb, c)), (be._h, 0x80000001, (e, None, None, None, None)),
                           (be._h, 0, (e + 2, m, r, nb, c)), (be._h, 0, (e, m + 1, r, nb, c)), (be._h, 0, (e, m, r + 2, nb, c)),
                           (be._h, 0, (e, m, r, nb + 3, c)), (be._h, 0, (e, m, r, nb, c + 2)), (be._h, 0, (e, m, None, nb, c)),
                           (be._h, 1, (None, None, None, nb, None))):
        assert lib.sb_batch_graph_device(h, flags, *[vp(p) for p in args]) == 1, (flags, args)
    assert b"row_ptr" in lib.sb_batch_last_error(be._h)
    be.sync()
    assert all((x.cpu().numpy() == 77).all() for x in outs), "no output was touched"
    assert lib.sb_batch_graph_device(be._h, 0, None, None, None, None, None) == 0, "nothing wanted: nothing done"
    with pytest.raises(ValueError):
        be.graph(adjacency=(False, True))
    with pytest.raises(ValueError):
        be.graph(ends=torch.zeros(5, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        be.graph(material=torch.zeros((1, 64, 5), dtype=torch.int32, device="cuda"))
    assert lib.sb_batch_graph_device(be._h, 1, vp(e), vp(m), vp(r), vp(nb), vp(c)) == 0
    be.sync()
    assert outs[4].cpu().numpy().tolist() == [30, 14, 8, 0]
    be.destroy()


def test_kernel_resources(sb):
    """9: no scratch; the info keys"""
    be = sb.BatchEngine(n_scenes=1, max_particles=1024, max_beams=4096)
    assert be.info("graph_kernel_scratch_bytes") == 0 and 0 < be.info("graph_kernel_vgprs") <= 128
    assert be.info("graph_count_words") == 4 and be.info("graph_material_words") == 5
    assert be.info("graph_lds_bytes") == (8192 + 2 * 1024 + 1 + 128 + 3) * 4 <= 65536
    be.destroy()
