"""What the GPU tests of the engine's four whole-scene reports share (tests/test_gpu_{summary,bodies,contacts,body_summary}.py), in
the manner of batch_harness.py: the engine constructor and the body of their read-only tests."""
from test_gpu_parity import assert_same

FLAGS = ("acc_dirty_tiles", "plastic_tiles", "grid_schedule", "substeps_done")


def engine(sb, buf, bounds, **kw):
    """an engine at the scene's capacity with the scene uploaded"""
    eng = sb.Engine(bounds_size=bounds, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, **kw)
    eng.write_buffers(buf)
    return eng


def in_place(got, given, shape):
    """`got` is what a report returns for the tensor `given` that it wrote into: `given` itself where it has the documented
    `shape`, else a view of that shape over the same storage"""
    if tuple(given.shape) == tuple(shape):
        return got is given
    return tuple(got.shape) == tuple(shape) and got.data_ptr() == given.data_ptr() and got.untyped_storage().data_ptr() == given.untyped_storage().data_ptr()


def read_only(sb, what, mk, kw, make, calls, keys=(), after=None):
    """frame, the report calls, frame == frame, frame: the read-back byte for byte, the summary row and its counts, the promise
    flags, the schedule and the info keys `keys`.  make(sb, case, **kw): the file's engine; calls(eng, case): the report calls;
    after(eng, case): the file's own assertions on each engine before it is destroyed."""
    if mk is None:   # a quiet lattice: the hybrid runs blocked launches under SB_COLLIDE_GRID
        buf = sb.scenes.lattice_buffers(128, 96, d=30.0, origin=(300.0, 900.0), jitter=1.0, layout=2, velocity=(0.4, -1.0))
        case = dict(buf=buf, bounds=6000.0)
    else:
        case = mk(sb)
    out = {}
    for k in ("plain", "read"):
        eng = make(sb, case, **kw)
        eng.frame()
        if k == "read":
            calls(eng, case)
        eng.frame()
        row, counts = eng.summary(counts=True)
        out[k] = (eng.load_buffers(case["buf"].copy()), row.cpu().numpy().tobytes(), counts.cpu().numpy().tolist(),
                  [eng.info(x) for x in FLAGS + tuple(keys)])
        if what == "hybrid":
            assert eng.info("hybrid_launches") > 0
        if after is not None:
            after(eng, case)
        eng.destroy()
    assert_same(out["read"][0], out["plain"][0], what)
    assert out["read"][1:] == out["plain"][1:], (what, out["read"][2:], out["plain"][2:])
