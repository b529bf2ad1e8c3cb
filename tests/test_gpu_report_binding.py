"""The two sides of the C ABI of the engine's reports against each other: what the host variant copies out through
its mirror is, byte for byte, what the device variant writes -- into tensors of the documented shape (which come back as the same
objects), into flat, oversized tensors (which come back as views of the documented shape over the same storage, the surplus
untouched) and through raw device pointers.  One small scene for all six: an 8 x 6 lattice with one beam removed by a delete pass
and one break pending, in an engine of 64 particles and 128 beams, the particles large enough that neighbours touch.  The reports'
own files check the values; that host and device variant agree is also asserted there on their scenes
(test_ordering_and_host_variant of test_gpu_summary.py and test_gpu_bodies.py, and their like)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAXP, MAXB, ROWS, PAIRS = 64, 128, 4, 8
PATTERN = 0x5A     # what every buffer holds before a call
SURPLUS = 5        # elements a flat tensor has too many


@pytest.fixture(scope="module")
def scene(sb):
    """(engine, labels of its bodies on the device): nothing below changes the engine's state"""
    p, b = sb.scenes.rectangle(100.0, 100.0, 30.0, 8, 6, 50.0, 700.0, 0.2, 1.0e9, anti_diagonal=False, layout=2)
    pv = np.zeros((len(p), 6), "<f4")
    pv[:, :2] = p
    buf = sb.Buffers(2, MAXP, MAXB)
    buf.set_scene(pv, b)
    eng = sb.Engine(bounds_size=1000.0, particle_radius=16.0, layout=2, max_particles=MAXP, max_beams=MAXB)
    eng.write_buffers(buf)
    _, c = eng.cut(sb.cut_shapes(segments=[(115.0, 90.0, 115.0, 105.0)]))     # the first row's first beam along x ...
    assert c.tolist() == [len(b), 1, 1, 0]
    eng.delete_pass()                                                         # ... is removed
    _, c = eng.cut(sb.cut_shapes(segments=[(95.0, 145.0, 105.0, 145.0)]))      # the first column's second beam along y is pending
    assert c.tolist() == [len(b) - 1, 1, 1, 0]
    row, counts = eng.summary_host()
    assert counts[:4].tolist() == [48, len(b) - 1, 1, 1]
    labels = eng.bodies(counts=False)[0]
    yield eng, labels
    eng.destroy()


KNIFE = dict(segments=[(205.0, 0.0, 205.0, 1000.0)])     # between two columns: a dry run hits eleven beams

# name: (the outputs (name, shape, dtype) in the order both calls below return them, the host variant, the device variant into `b`)
REPORTS = {
    "summary": ((("out", (24,), "float32"), ("counts", (8,), "int64")),
                lambda sb, e, lab: e.summary_host(),
                lambda sb, e, lab, b: e.summary(out=b[0], counts=b[1])),
    "bodies": ((("labels", (MAXP,), "int32"), ("sizes", (MAXP, 2), "int32"), ("counts", (4,), "int64")),
               lambda sb, e, lab: e.bodies_host(),
               lambda sb, e, lab, b: (lambda l, c, s: (l, s, c))(*e.bodies(labels=b[0], sizes=b[1], counts=b[2]))),
    "contacts": ((("touch", (MAXP, 4), "int32"), ("counts", (4,), "int64"), ("pairs", (PAIRS, 2), "int32")),
                 lambda sb, e, lab: e.contacts_host(labels=lab.cpu().numpy(), pairs=PAIRS),
                 lambda sb, e, lab, b: e.contacts(labels=lab, pairs=PAIRS, touch=b[0], counts=b[1], out=b[2])),
    "body_summary": ((("out", (ROWS, 24), "float32"), ("counts", (ROWS, 8), "int64"), ("rank", (MAXP,), "int32")),
                     lambda sb, e, lab: e.body_summary_host(rows=ROWS),
                     lambda sb, e, lab, b: e.body_summary(rows=ROWS, out=b[0], counts=b[1], rank=b[2])),
    "graph": ((("ends", (MAXB, 2), "int32"), ("row_ptr", (MAXP + 1,), "int64"), ("nbr", (2 * MAXB, 2), "int32"), ("counts", (4,), "int64")),
              lambda sb, e, lab: e.graph_host(),
              lambda sb, e, lab, b: e.graph(ends=b[0], adjacency=(b[1], b[2]), max_half_edges=2 * MAXB, counts=b[3])),
    "cut": ((("hit", (MAXB,), "uint8"), ("counts", (4,), "int64")),       # (hit is not written where no beam is: the pattern stays)
            lambda sb, e, lab: e.cut(sb.cut_shapes(**KNIFE), dry_run=True, hit=np.full(MAXB, PATTERN, np.uint8)),
            lambda sb, e, lab, b: e.cut(on_device(sb.cut_shapes(**KNIFE)), dry_run=True, hit=b[0], counts=b[1])),
}


def on_device(shapes):
    import torch
    return torch.from_numpy(shapes.view(np.int32)).cuda()


def filled(n, dtype):
    import torch
    return torch.full((n * np.dtype(dtype).itemsize,), PATTERN, dtype=torch.uint8, device="cuda").view(getattr(torch, dtype))


@pytest.mark.parametrize("name", sorted(REPORTS))
def test_host_and_device_variant_write_the_same_bytes(sb, scene, name):
    import torch
    eng, labels = scene
    outs, host, device = REPORTS[name]
    want = [np.ascontiguousarray(x).tobytes() for x in host(sb, eng, labels)]
    sizes = [int(np.prod(shape)) for _, shape, _ in outs]
    assert [len(w) for w in want] == [n * np.dtype(dtype).itemsize for n, (_, _, dtype) in zip(sizes, outs)]
    if name == "cut":
        assert np.frombuffer(want[1], np.int64).tolist() == [116, 11, 0, 0] and want[0].count(bytes([PATTERN])) == MAXB - 117
    print(name, {o[0]: len(w) for o, w in zip(outs, want)})

    def same(got, how):
        for (what, _, _), g, w in zip(outs, got, want):
            assert g.cpu().numpy().tobytes() == w, "%s, %s: %s differs from the host variant's" % (name, how, what)

    # tensors of the documented shape: the same objects come back
    exact = [filled(n, dtype).view(shape) for n, (_, shape, dtype) in zip(sizes, outs)]
    got = device(sb, eng, labels, exact)
    assert all(g is x for g, x in zip(got, exact)), name
    same(got, "tensors of the shape")
    # flat and too large: views of the shape over the same storage, nothing written behind them
    flat = [filled(n + SURPLUS, dtype) for n, (_, _, dtype) in zip(sizes, outs)]
    got = device(sb, eng, labels, flat)
    for (what, shape, _), g, x in zip(outs, got, flat):
        assert tuple(g.shape) == shape and g.data_ptr() == x.data_ptr() and g.untyped_storage().data_ptr() == x.untyped_storage().data_ptr(), (name, what)
    same(got, "flat tensors")
    assert all((x[n:].view(torch.uint8) == PATTERN).all() for n, x in zip(sizes, flat)), name + ": the surplus was written"
    # raw pointers: no tensor, so nothing orders the streams but the two waits here
    raw = [filled(n, dtype) for n, (_, _, dtype) in zip(sizes, outs)]
    torch.cuda.synchronize()
    got = device(sb, eng, labels, [x.data_ptr() for x in raw])
    assert list(got) == [x.data_ptr() for x in raw], name
    eng.sync()
    same(raw, "device pointers")
