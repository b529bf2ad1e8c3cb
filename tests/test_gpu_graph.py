"""Engine.graph (sb_graph_device / sb_graph) on the GPU, on the atomic, tiled and blocked layouts, every comparison
np.array_equal against tests/graph_ref.py on what load_buffers returns: a 40 x 40 lattice; the lattice after cut() and a delete
pass, and with skip_pending before the pass; after a plan-keeping re-upload that removed beams; with max_half_edges below the
total; a 600 x 600 lattice whose row_ptr crosses the scan's block-sum loop; the host copy against the device call; read-only;
argument errors; no scratch."""
import ctypes

import numpy as np
import pytest

import bodies_cases as bc
import graph_ref as ref
import report_harness as rh
from test_gpu_bodies import PATHS
from test_gpu_parity import OFF, assert_same

pytestmark = pytest.mark.gpu

W = 40
BOUNDS = 4000.0
X_CUT = 100.0 + 30.0 * 19.5     # between the lattice's columns 19 and 20


def lattice(sb, w=W, h=W, slack=5):
    return sb.scenes.lattice_buffers(w, h, d=30.0, origin=(100.0, 100.0), strain_limit=0.5, layout=2, slack=slack)


def want(buf, H=None, drop=()):
    """the restatement in the engine's shapes: (ends, row_ptr int64, nbr [H, 2], counts int64)"""
    g = ref.graph_ref(buf, drop=drop)
    H = 2 * buf.max_beams if H is None else H
    nbr = np.full((H, 2), -1, np.int32)
    k = min(H, 2 * buf.max_beams)
    nbr[:k] = g.nbr[:k]
    return g.ends, g.row_ptr.astype(np.int64), nbr, g.counts.astype(np.int64)


def device_graph(eng, H=None, **kw):
    """Engine.graph into pattern-filled tensors, with eight more rows of nbr than it may write: as numpy, the guard rows apart"""
    import torch
    rows = 2 * eng.max_beams if H is None else H
    ends = torch.full((eng.max_beams, 2), -1515870811, dtype=torch.int32, device="cuda")
    row_ptr = torch.full((eng.max_particles + 1,), -77, dtype=torch.int64, device="cuda")
    nbr = torch.full((rows + 8, 2), -1515870811, dtype=torch.int32, device="cuda")
    counts = torch.full((4,), -77, dtype=torch.int64, device="cuda")
    out = eng.graph(ends=ends, adjacency=(row_ptr, nbr), max_half_edges=rows, counts=counts, **kw)
    assert out[0] is ends and out[1] is row_ptr and out[3] is counts and rh.in_place(out[2], nbr, (rows, 2))
    got = [x.cpu().numpy() for x in (ends, row_ptr, nbr, counts)]
    assert (got[2][rows:] == -1515870811).all(), "rows at or behind max_half_edges are not written"
    got[2] = got[2][:rows]
    return tuple(got)


def same(got, exp, what):
    for name, x, y in zip(("ends", "row_ptr", "nbr", "counts"), got, exp):
        assert x.dtype == y.dtype and np.array_equal(x, y), "%s: %s differs" % (what, name)


def check(eng, buf, what, H=None, **kw):
    now = eng.load_buffers(buf.copy())
    got = device_graph(eng, H, **kw)
    print(what, "counts", got[3].tolist())
    same(got, want(now, H), what)
    return now, got


def without(buf, keep):
    """the scene without the beams whose `keep` is False (an upload that only removes beams)"""
    return bc.without(buf, keep)


@pytest.mark.parametrize("what,kw", PATHS, ids=[p[0] for p in PATHS])
def test_lattice_cut_and_reuploaded(sb, what, kw):
    buf = lattice(sb)
    eng = rh.engine(sb, buf, BOUNDS, collision_mode=OFF, **kw)
    # the lattice as uploaded; every half-edge, then fewer rows than there are
    _, g = check(eng, buf, what + ", uploaded")
    B = buf.beam_count
    assert g[3].tolist() == [B, W * W, 6, W + 1] and g[1][-1] == 2 * B      # (interior degree 6: +y, +x and one diagonal)
    _, short = check(eng, buf, what + ", 1000 rows", H=1000)
    assert np.array_equal(short[1], g[1]) and np.array_equal(short[2], g[2][:1000]), "row_ptr is complete, nbr is the head of the list"
    _, ample = check(eng, buf, what + ", more rows than half-edges", H=2 * B + 50)
    assert (ample[2][2 * B:] == -1).all()
    # a knife between two columns: pending, the cut beams are still listed; skip_pending is what the delete pass leaves
    hit, c = eng.cut(sb.cut_shapes(segments=[(X_CUT, 0.0, X_CUT, 2000.0)]), hit=True)
    hit = np.asarray(hit).astype(bool)
    assert hit.sum() == int(c[1]) == 2 * W - 1                               # (W beams in x and W - 1 diagonals cross)
    now, pending = check(eng, buf, what + ", cut pending")
    same(pending, g, what + ": a pending cut is still listed")
    skipped = device_graph(eng, skip_pending=True)
    same(skipped, want(now, drop=np.flatnonzero(hit)), what + ", skip_pending")
    assert skipped[3][0] == B - hit.sum() and (skipped[0][hit] == -1).all()
    eng.delete_pass()
    _, after = check(eng, buf, what + ", after the delete pass")
    same(skipped, after, what + ": skip_pending == after the pass")
    same(device_graph(eng, skip_pending=True), after, what + ": no flag is pending after the pass")
    # the host copy against the device call
    host = eng.graph_host()
    same(host, after, what + ", sb_graph == sb_graph_device")
    same(eng.graph_host(max_half_edges=100)[:2] + (eng.graph_host(max_half_edges=100)[2],), (after[0], after[1], after[2][:100]), what + ", host, 100 rows")
    eng.destroy()
    # a plan-keeping re-upload that removed beams (no delete pass runs)
    rec = buf.beams[buf.mapping[buf.max_particles:buf.max_particles + B].astype(np.int64)]
    left = buf.particles[:, 0] < np.float32(X_CUT)
    keep = left[rec["a"].astype(np.int64)] == left[rec["b"].astype(np.int64)]
    cut = without(buf, keep)
    eng = rh.engine(sb, buf, BOUNDS, collision_mode=OFF, **kw)
    check(eng, buf, what + ", whole again")
    eng.write_buffers(cut)
    assert eng.info("uploads_edited") == 1
    _, g2 = check(eng, cut, what + ", re-uploaded without the crossing beams")
    assert g2[3][0] == B - (2 * W - 1) == cut.beam_count
    assert eng.info("graph_table_build_us") > 0
    eng.destroy()


def test_row_ptr_past_256_scan_blocks(sb):
    """600 x 600: 360 001 words of row_ptr are 352 scan blocks, so the block sums take the single workgroup's loop twice"""
    buf = lattice(sb, 600, 600, slack=0)
    eng = rh.engine(sb, buf, 20000.0, collision_mode=OFF)
    assert (buf.max_particles + 1 + 1023) // 1024 > 256
    _, g = check(eng, buf, "600 x 600")
    assert g[3].tolist() == [buf.beam_count, 360000, 6, 601] and g[1][-1] == 2 * buf.beam_count
    eng.destroy()


def test_read_only_outputs_and_errors(sb):
    import torch
    buf = lattice(sb, 12, 12)
    out = {}
    for k in ("plain", "read"):
        eng = rh.engine(sb, buf, BOUNDS, collision_mode=OFF)
        eng.frame()
        if k == "read":
            device_graph(eng)
            device_graph(eng, skip_pending=True)
            eng.graph_host()
        eng.frame()
        out[k] = eng.load_buffers(buf.copy())
        if k == "plain":
            eng.destroy()
    assert_same(out["read"], out["plain"], "frame, graph, frame == frame, frame")
    # parts of the outputs
    full = device_graph(eng)
    e, r, n, c = eng.graph()
    assert r is None and n is None and np.array_equal(e.cpu().numpy(), full[0]) and np.array_equal(c.cpu().numpy(), full[3])
    e, r, n, c = eng.graph(ends=False, adjacency=True, max_half_edges=0, counts=False)
    assert e is None and n is None and c is None and np.array_equal(r.cpu().numpy(), full[1])
    e, r, n, c = eng.graph(ends=False, adjacency=True, counts=False)
    assert np.array_equal(n.cpu().numpy(), full[2])
    # errors: nothing is enqueued
    lib = sb.engine.load_library()
    vp = ctypes.c_void_p
    outs = [torch.full((k,), 77, dtype=dt, device="cuda") for k, dt in ((eng.max_beams * 2, torch.int32), (eng.max_particles + 1, torch.int64),
                                                                          (64, torch.int32), (4, torch.int64))]
    pe, pr, pn, pc = (x.data_ptr() for x in outs)
    torch.cuda.synchronize()

    def opts(flags=0, H=32, size=None, reserved=0):
        o = sb.engine.SbGraphOptions()
        o.struct_size = ctypes.sizeof(o) if size is None else size
        o.flags, o.max_half_edges = flags, H
        o.reserved[1] = reserved
        return o

    for h, o, args in ((None, opts(), (pe, pr, pn, pc)), (eng._h, opts(flags=2), (pe, pr, pn, pc)), (eng._h, opts(size=8), (pe, pr, pn, pc)),
                       (eng._h, opts(reserved=1), (pe, pr, pn, pc)), (eng._h, opts(), (pe + 2, pr, pn, pc)), (eng._h, opts(), (pe, pr + 4, pn, pc)),
                       (eng._h, opts(), (pe, pr, pn + 1, pc)), (eng._h, opts(), (pe, pr, pn, pc + 4)), (eng._h, opts(), (pe, None, pn, pc)),
                       (eng._h, opts(H=0), (pe, pr, pn, pc))):
        assert lib.sb_graph_device(h, ctypes.byref(o), *[vp(p) for p in args]) == 1, (o.flags, args)
    eng.sync()
    assert all((x.cpu().numpy() == 77).all() for x in outs), "no output was touched"
    with pytest.raises(ValueError):
        eng.graph(adjacency=(False, True))
    fresh = sb.Engine(bounds_size=BOUNDS, layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=OFF)
    assert lib.sb_graph_device(fresh._h, None, vp(pe), None, None, None) == 5, "SB_ERR_STATE before an upload"
    fresh.destroy()
    assert eng.info("graph_kernel_scratch_bytes") == 0 and eng.info("graph_kernel_vgprs") > 0
    eng.destroy()
