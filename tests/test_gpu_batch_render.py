"""BatchEngine.render / render_scene (sb_batch_render_device / sb_batch_render_scene: one picture per scene, one launch) against
tests/render_ref.py's restatement of host/render.js on what load_scene returns.  The comparison is np.array_equal over whole
pictures: no tolerance, no pixel left out.  Scenes come from tests/batch_cases.py; tests/test_batch_render_cpu.py asserts on the
CPU that their pictures are not black."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
from batch_harness import apply_to_batch, make_batch, upload_each  # noqa: E402
from render_ref import render_ref  # noqa: E402

pytestmark = pytest.mark.gpu

OFF, ALLPAIRS, GRID = 0, 1, 2
S0, R0 = 1000.0, 10.0


class Refs:
    """render_ref(be.load_scene(i, template), res, S, r), remembered per scene CONTENT (a replicated batch holds the same scene
    many times; every scene is still loaded and compared)."""

    def __init__(self):
        self.seen = {}

    def picture(self, be, i, template, res, S=S0, r=R0):
        if template is None:
            return np.zeros((res, res, 3), np.uint8)          # never uploaded: black by definition
        buf = be.load_scene(i, template.copy())
        key = (buf.metadata.tobytes(), buf.mapping.tobytes(), buf.particles.tobytes(), buf.beams.tobytes(), res, S, r)
        if key not in self.seen:
            self.seen[key] = render_ref(buf, res, S, r)
        return self.seen[key]


def assert_pictures(be, templates, res, refs, what, S=None, r=None, prefill=None):
    """render() of the whole batch against the reference of every scene; returns the pictures (numpy)."""
    import torch
    n = be.n_scenes
    out = None
    if prefill is not None:
        out = torch.full((n, res, res, 3), prefill, dtype=torch.uint8, device="cuda:%d" % be.device)
    got = be.render(res, bounds_size=S, particle_radius=r, out=out)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, res, res, 3) and got.device.type == "cuda"
    be.sync()
    g = got.cpu().numpy()
    for i in range(n):
        want = refs.picture(be, i, templates[i], res, S0 if S is None else S, R0 if r is None else r)
        bad = int((g[i] != want).any(axis=-1).sum())
        print("%s: scene %d at %d^2: %d pixels differ, %d not black" % (what, i, res, bad, int((want != 0).any(axis=-1).sum())))
        assert np.array_equal(g[i], want), "%s: scene %d at %d^2: %d pixels differ" % (what, i, res, bad)
    return g


@pytest.mark.parametrize("layout", [1, 2])
def test_default_scene_replicated_over_64_scenes(sb, layout):
    case = bc.case_default(sb, layout)
    buf = case["bufs"][0]
    be = make_batch(sb, case, n=64)
    be.write_scene(buf)
    eng = sb.Engine(layout=layout, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=GRID)
    eng.write_buffers(buf)
    refs, seen = Refs(), {}
    done = 0
    for frames in (0, 1, 3):
        be.frame(frames - done)
        for _ in range(frames - done):
            eng.frame()
        done = frames
        for res in (64, 85, 128):
            g = assert_pictures(be, [buf] * 64, res, refs, "default v%d after %d frames" % (layout, frames))
            assert int((g[0] != 0).any(axis=-1).sum()) > 100
            assert np.array_equal(g[0], eng.render(res)), "scene 0 differs from Engine.render after %d frames at %d" % (frames, res)
            assert np.array_equal(be.render_scene(63, res), g[63])
            seen[(frames, res)] = g[0]
    for res in (64, 85, 128):
        assert not np.array_equal(seen[(0, res)], seen[(1, res)]) and not np.array_equal(seen[(1, res)], seen[(3, res)])
    assert be.info("render_bands") >= 1 and be.info("render_kernel_scratch_bytes") == 0 and be.info("render_kernel_vgprs") > 0
    assert 0 < be.info("render_lds_bytes") <= 160 * 1024
    be.render(64)
    assert be.info("render_bands") == 1 and be.info("render_lds_bytes") > 64 * 64 * 4
    eng.destroy()
    be.destroy()


def _hetero(sb):
    case = bc.case_hetero(sb)
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    for op in case["program"]:
        apply_to_batch(be, op)
    return case, be


def test_heterogeneous_batch_after_a_partial_frame(sb):
    """Default scene, 12 x 12 lattice, the 1024-particle lattice, two particles, the empty scene and one never uploaded, after
    2 frames + 7 substeps (strain / stress of a partial call), into a tensor pre-filled with 0xAB."""
    case, be = _hetero(sb)
    assert case["program"][-1] == ("step", 7)
    refs = Refs()
    for res in (64, 128, 256):
        g = assert_pictures(be, case["bufs"], res, refs, "heterogeneous", prefill=0xAB)
        assert not g[4].any() and not g[5].any()                 # empty and never uploaded: black, and written
        assert all(g[i].any() for i in range(4))
    assert be.info("render_bands") > 1                           # 256^2 does not fit one band
    be.destroy()


def test_breaking_lattices_after_each_frame(sb):
    case = bc.case_break(sb)
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    refs, colours, counts = Refs(), set(), []
    for k in range(3):
        be.frame(1)
        g = assert_pictures(be, case["bufs"], 128, refs, "break, frame %d" % (k + 1))
        colours |= {tuple(c) for c in np.unique(g.reshape(-1, 3), axis=0)}
        counts.append([be.load_scene(i, b.copy()).beam_count for i, b in enumerate(case["bufs"])])
    assert len(colours) > 3, colours
    assert counts[-1][4] < case["bufs"][4].beam_count            # beams were removed: the slots compacted
    be.destroy()


def test_permuted_mapping_and_coincident_particles(sb):
    case = bc.case_mapping(sb)
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    refs = Refs()
    for k in range(2):
        for res in (64, 128):
            assert_pictures(be, case["bufs"], res, refs, "mapping, frame %d" % k)
        be.frame(1)
    be.destroy()


@pytest.mark.parametrize("res", [256, 333, 1024])
def test_bands(sb, res):
    case = bc.case_default(sb, 1)
    buf = case["bufs"][0]
    be = make_batch(sb, case, n=3)
    be.write_scene(buf)
    be.frame(1)
    refs = Refs()
    assert_pictures(be, [buf] * 3, res, refs, "bands")
    assert be.info("render_bands") > 1
    if res != 1024:
        for S, r in ((400.0, 25.0), (1000.0, 120.0)):
            g = assert_pictures(be, [buf] * 3, res, refs, "bands, wide primitives (%g, %g)" % (S, r), S=S, r=r)
            assert int((g[0] != 0).any(axis=-1).sum()) > 1000   # (over 1000 at 64^2 already: test_batch_render_cpu.py)
    be.destroy()


@pytest.mark.parametrize("res", [64, 85])
def test_wide_primitives_in_one_band(sb, res):
    case = bc.case_default(sb, 2)
    buf = case["bufs"][0]
    be = make_batch(sb, case, n=2)
    be.write_scene(buf)
    be.frame(1)
    refs = Refs()
    for S, r in ((400.0, 25.0), (1000.0, 120.0)):
        assert_pictures(be, [buf] * 2, res, refs, "wide primitives (%g, %g)" % (S, r), S=S, r=r)
    assert be.info("render_bands") == 1
    be.destroy()


def test_wide_primitives_across_bands_at_1024(sb):
    case = bc.case_default(sb, 1)
    buf = case["bufs"][0]
    be = make_batch(sb, case, n=1)
    be.write_scene(buf)
    be.frame(1)
    assert_pictures(be, [buf], 1024, Refs(), "1024^2, wide primitives", S=1000.0, r=120.0)
    assert be.info("render_bands") > 1
    be.destroy()


@pytest.mark.parametrize("res", [64, 256])
def test_particles_outside_the_box_and_non_finite_coordinates(sb, res):
    case = bc.case_default(sb, 1)
    buf = case["bufs"][0]
    be = make_batch(sb, case, n=3)
    be.write_scene(buf)
    be.frame(1)
    p, _, _ = be.state_tensors()
    clean = be.render(res).cpu().numpy()
    p[1, 5, 0], p[1, 6, 1], p[1, 40, 0], p[1, 41, 1] = 1500.0, -300.0, 1e30, -1e30       # outside the box, near and far
    p[2, 3, 0], p[2, 7, 1], p[2, 20, 0], p[2, 60, 1] = float("nan"), float("nan"), float("inf"), float("-inf")
    be.write_particles_device(p)
    refs = Refs()
    g = assert_pictures(be, [buf] * 3, res, refs, "outside / non-finite")
    assert np.array_equal(g[0], clean[0]) and not np.array_equal(g[1], clean[1]) and not np.array_equal(g[2], clean[2])
    got = be.load_scene(2, buf.copy())
    assert np.isnan(got.particles[3, 0]) and np.isinf(got.particles[20, 0])              # the reference did see them
    be.destroy()


def test_first_and_count_write_exactly_count_pictures(sb):
    import torch
    case = bc.case_default(sb, 2)
    buf = case["bufs"][0]
    be = make_batch(sb, case, n=8)
    be.write_scene(buf)
    for i in range(8):                       # different gravity per scene: eight different pictures
        be.set_physics_constants(np.array([0.05 * i, -0.5, 0.5, 0.2, 0.5, 0.1, 0.001, 2.0], "f4"), first=i, count=1)
    be.frame(2)
    refs = Refs()
    for res in (64, 85):
        nb = res * res * 3
        raw = torch.full((5 * nb + 1,), 0xAB, dtype=torch.uint8, device="cuda:0")
        out = raw[1:]                         # a base address that is not a multiple of 4
        got = be.render(res, first=2, count=3, out=out)
        assert tuple(got.shape) == (3, res, res, 3) and got.data_ptr() == out.data_ptr()
        be.sync()
        h = raw.cpu().numpy()
        assert h[0] == 0xAB and (h[1 + 3 * nb:] == 0xAB).all()
        pics = h[1:1 + 3 * nb].reshape(3, res, res, 3)
        for k in range(3):
            assert np.array_equal(pics[k], refs.picture(be, 2 + k, buf, res)), (res, k)
        assert not np.array_equal(pics[0], pics[1]) and not np.array_equal(pics[1], pics[2])
        last = be.render(res, first=7)
        assert tuple(last.shape) == (1, res, res, 3)
        assert np.array_equal(last.cpu().numpy()[0], refs.picture(be, 7, buf, res))
    be.destroy()


def test_a_render_only_reads(sb):
    case = bc.case_break(sb)
    runs = []
    for render in (True, False):
        be = make_batch(sb, case)
        upload_each(be, case["bufs"])
        be.frame(1)
        be.step(5)                            # break flags pending, no delete pass yet
        if render:
            be.render(128)
            be.render(333, bounds_size=400.0, particle_radius=25.0)
            be.render_scene(4, 64)
        be.frame(1)
        p, b, a = be.state_tensors()
        be.sync()
        runs.append(([t.cpu().numpy().view(np.uint8 if t.element_size() == 1 else np.uint32) for t in (p, b, a)],
                     [be.load_scene(i, buf.copy()) for i, buf in enumerate(case["bufs"])]))
        be.destroy()
    for x, y in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(x, y)
    for i, (x, y) in enumerate(zip(runs[0][1], runs[1][1])):
        bc.assert_same(x, y, "scene %d" % i)
    assert any(x.beam_count < buf.beam_count for x, buf in zip(runs[0][1], case["bufs"]))   # flags were pending and acted on


def test_stream_ordering_against_torchs_current_stream(sb):
    case = bc.case_default(sb, 1)
    buf = case["bufs"][0]
    be = make_batch(sb, case, n=256)
    be.write_scene(buf)
    be.frame(2)
    got = be.render(128).cpu().numpy()        # no sync(): torch's current stream is ordered behind the render
    want = Refs().picture(be, 0, buf, 128)
    assert want.any()
    for i in range(256):
        assert np.array_equal(got[i], want), i
    be.destroy()


def test_errors(sb):
    import torch
    case, be = _hetero(sb)
    L = sb.batch.load_library()
    n = be.n_scenes

    def c_render(res, first, count, ptr, size=None):
        o = sb.batch.SbBatchRenderOptions()
        o.struct_size = ctypes.sizeof(o) if size is None else size
        o.resolution, o.first, o.count = res, first, count
        return L.sb_batch_render_device(be._h, ctypes.byref(o), ctypes.c_void_p(ptr))

    ok = torch.empty(n * 64 * 64 * 3, dtype=torch.uint8, device="cuda:0")
    assert c_render(64, 0, 0, ok.data_ptr()) == 0
    assert c_render(1025, 0, 1, ok.data_ptr()) == 1 and b"1025" in L.sb_batch_last_error(be._h)
    assert c_render(64, 0, n + 1, ok.data_ptr()) == 1 and c_render(64, n, 0, ok.data_ptr()) == 1
    assert c_render(64, 2, n - 1, ok.data_ptr()) == 1 and c_render(64, 0xFFFFFFFF, 2, ok.data_ptr()) == 1
    assert c_render(64, 0, 1, None) == 1 and c_render(64, 0, 1, ok.data_ptr(), size=8) == 1
    host = np.empty(64 * 64 * 3, np.uint8)
    o = sb.batch.SbBatchRenderOptions()
    o.struct_size, o.resolution = ctypes.sizeof(o), 64
    hp = host.ctypes.data_as(ctypes.c_void_p)
    assert L.sb_batch_render_scene(be._h, 0, ctypes.byref(o), hp, host.nbytes - 1) == 1
    assert L.sb_batch_render_scene(be._h, n, ctypes.byref(o), hp, host.nbytes) == 1
    assert L.sb_batch_render_scene(be._h, 0, ctypes.byref(o), None, host.nbytes) == 1
    assert L.sb_batch_render_scene(be._h, 0, None, hp, host.nbytes) == 0         # NULL options: all defaults (64^2)
    assert L.sb_batch_render_scene(be._h, 5, ctypes.byref(o), hp, host.nbytes) == 5
    be.sync()

    for bad in (lambda: be.render(1025), lambda: be.render(64, first=1, count=n),
                lambda: be.render(64, out=torch.empty(n * 64 * 64 * 3, dtype=torch.uint8)),                      # wrong device
                lambda: be.render(64, out=torch.empty(n * 64 * 64 * 3, dtype=torch.int8, device="cuda:0")),      # wrong dtype
                lambda: be.render(64, out=torch.empty(n * 64 * 64 * 3 - 1, dtype=torch.uint8, device="cuda:0"))):  # short
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(sb.EngineError) as ei:
        be.render_scene(5, 64)
    assert ei.value.status == 5 and "never uploaded" in str(ei.value)
    assert not be.render_scene(4, 64).any()                                      # the empty scene WAS uploaded: black
    with pytest.raises(sb.EngineError) as ei:
        be.info("render_nothing")
    assert ei.value.status == 1
    be.destroy()
