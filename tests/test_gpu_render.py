"""sb_render on the GPU: the picture of host/render.js (tests/render_ref.py restates it) of the state sb_load_buffers returns, byte
for byte, on every schedule the engine runs, after delete passes and re-uploads, at any resolution; and a render changes nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

from render_ref import render_ref
from test_gpu_parity import ALLPAIRS, ATOMIC, GRID, OFF, TILED, assert_same
from test_gpu_reupload import breaking_lattice, moved, without

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def f32(x):
    return float(np.float32(x))


def same_picture(eng, template, bounds, res=512, bounds_size=None, particle_radius=None, radius=10.0, what=""):
    """sb_render == render_ref(the state sb_load_buffers returns now)."""
    got = eng.render(res, bounds_size, particle_radius)
    state = eng.load_buffers(template.copy())
    exp = render_ref(state, res, f32(bounds) if bounds_size is None else bounds_size,
                     f32(radius) if particle_radius is None else particle_radius)
    assert got.shape == (res, res, 3) and got.dtype == np.uint8
    if not np.array_equal(got, exp):
        bad = np.nonzero((got != exp).any(axis=2))
        raise AssertionError("%s: %d of %d pixels differ, first (row %d, col %d): %s vs %s" % (
            what, bad[0].size, res * res, bad[0][0], bad[1][0], got[bad[0][0], bad[1][0]], exp[bad[0][0], bad[1][0]]))
    return got, state


def engine(sb, buf, bounds=1000.0, **kw):
    eng = sb.Engine(bounds_size=bounds, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, **kw)
    eng.write_buffers(buf)
    return eng


@pytest.mark.parametrize("mode,path", [(ALLPAIRS, ATOMIC), (GRID, 0)])
def test_default_scene_frames(sb, mode, path):
    buf = sb.scenes.default_buffers(1, 256, 512)
    eng = engine(sb, buf, collision_mode=mode, path=path)
    pics = [same_picture(eng, buf, 1000.0, what="0 frames")[0]]
    for n, total in ((2, 2), (88, 90)):
        for _ in range(n):
            eng.frame()
        pic, state = same_picture(eng, buf, 1000.0, what="%d frames" % total)
        pics.append(pic)
        if total == 2:   # ... and the picture of the oracle's state after 2 frames
            gold = sb.scenes.default_buffers(1)   # (the v1 snapshot's size check wants room for twice the counts)
            assert gold.load_snapshot(open(os.path.join(GOLDEN, "default_scene_v1_after_2_frames.snapshot"), "rb").read())
            assert np.array_equal(pic, render_ref(gold, 512, 1000.0, 10.0))
    eng.destroy()
    assert not np.array_equal(pics[0], pics[1]) and not np.array_equal(pics[1], pics[2])
    assert (pics[2] != 0).any(axis=2).sum() > 10000


@pytest.mark.parametrize("mode,path,kw,what", [
    (OFF, ATOMIC, {}, "atomic"),
    (GRID, ATOMIC, {}, "atomic, grid"),
    (OFF, TILED, {"block_substeps": 1}, "tiled, one substep per launch"),
    (OFF, TILED, {}, "blocked"),
    (GRID, TILED, {"tile_particles": 256}, "tiled, grid"),
])
def test_every_schedule(sb, mode, path, kw, what):
    first = breaking_lattice(sb)
    eng = engine(sb, first, 4000.0, collision_mode=mode, path=path, **kw)
    for _ in range(3):   # yields, breaks, delete passes
        eng.frame()
        same_picture(eng, first, 4000.0, 384, what=what)
    eng.step(5)          # mid-frame: strain / stress of a partial call
    same_picture(eng, first, 4000.0, 384, what=what + ", 5 more substeps")
    assert eng.counts()[1] < first.beam_count, "beams must have broken"
    eng.destroy()


def test_hybrid_quiet_lattice(sb):
    buf = sb.scenes.lattice_buffers(128, 96, d=30.0, origin=(300.0, 900.0), jitter=1.0, layout=2, velocity=(0.4, -1.0))
    eng = engine(sb, buf, 6000.0, collision_mode=GRID)
    eng.step(150)
    same_picture(eng, buf, 6000.0, 700, what="hybrid, 150")
    eng.step(150)
    same_picture(eng, buf, 6000.0, 700, what="hybrid, 300")
    assert eng.info("hybrid_launches") >= 30 and eng.info("hybrid_substeps") >= 200
    eng.destroy()


def pile_run(sb):
    buf, bounds = sb.scenes.config3_buffers(65536)
    eng = engine(sb, buf, bounds, collision_mode=GRID)
    for _ in range(3):
        eng.frame()
    same_picture(eng, buf, bounds, 1024, what="pile")
    eng.step(20)
    same_picture(eng, buf, bounds, 1024, what="pile, 20 more")
    info = {k: eng.info(k) for k in ("grid_classic_substeps", "grid_helper_launches", "substeps_done")}
    eng.destroy()
    return info


def test_grid_lagged_pile(sb):
    info = pile_run(sb)
    assert info["grid_helper_launches"] < info["substeps_done"], info


CLASSIC = r"""
import os, sys
root = sys.argv[1]   # the repository root
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import __graft_entry__ as ge
sb = ge.load_package()
from test_gpu_render import pile_run
info = pile_run(sb)
assert info["grid_classic_substeps"] == info["substeps_done"], info
print("classic ok", info)
"""


def test_grid_classic_pile(sb):
    env = dict(os.environ, SB_GRID_MODE="classic", SB_HYBRID="0")   # (read once per process: own process)
    p = subprocess.run([sys.executable, "-c", CLASSIC, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "classic ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("layout", [1, 2])
def test_reuploads(sb, layout):
    """Plan-keeping re-upload, an upload that cut beams, a shuffled mapping (plans again): the draw tables follow every upload."""
    first = breaking_lattice(sb, layout=layout)
    eng = engine(sb, first, 4000.0, collision_mode=GRID)
    eng.frame()
    same_picture(eng, first, 4000.0, 300, what="first")
    eng.write_buffers(moved(first, 7))
    assert eng.info("uploads_kept") == 1
    same_picture(eng, first, 4000.0, 300, what="kept plan, before a step")
    eng.frame()
    same_picture(eng, first, 4000.0, 300, what="kept plan")
    rng = np.random.default_rng(11)
    cut = without(moved(first, 8), rng.random(first.beam_count) >= 0.01)
    eng.write_buffers(cut)
    assert eng.info("uploads_edited") >= 1
    same_picture(eng, cut, 4000.0, 300, what="cut, before a step")
    for _ in range(2):
        eng.frame()
        same_picture(eng, cut, 4000.0, 300, what="cut")
    state = eng.load_buffers(cut.copy())
    from test_render_ref_cpu import shuffled
    sh = shuffled(state, 4)
    eng.write_buffers(sh)
    same_picture(eng, sh, 4000.0, 300, what="shuffled")
    eng.frame()
    same_picture(eng, sh, 4000.0, 300, what="shuffled, a frame")
    eng.destroy()


def test_config2_full_size(sb):
    buf = sb.scenes.lattice_buffers(1000, 1000, d=30.0, origin=(1000.0, 1000.0), jitter=1.0, layout=2)
    eng = engine(sb, buf, 32000.0, collision_mode=OFF)
    eng.step(20)
    pic, _ = same_picture(eng, buf, 32000.0, 1024, what="config 2")
    assert (pic != 0).any(axis=2).sum() > 100000
    eng.destroy()


def test_resolutions_overrides_errors(sb):
    from softbody_webgpu_amd.engine import EngineError
    buf = sb.scenes.default_buffers(2, 256, 512)
    eng = sb.Engine(layout=2, max_particles=256, max_beams=512)
    with pytest.raises(EngineError) as ex:
        eng.render(64)
    assert ex.value.status == 5   # SB_ERR_STATE
    eng.write_buffers(buf)
    eng.frame()
    for res in (1, 3, 4096):
        same_picture(eng, buf, 1000.0, res, what="resolution %d" % res)
    same_picture(eng, buf, 1000.0, 333, bounds_size=777.25, particle_radius=23.5, what="overrides")
    same_picture(eng, buf, 1000.0, 200, bounds_size=4000.0, what="bounds only")
    with pytest.raises(EngineError) as ex:
        eng.render(16385)
    assert ex.value.status == 1
    import ctypes
    lib = sb.engine.load_library()
    o = eng._render_options(64, None, None)
    small = np.zeros(64 * 64 * 3 - 1, np.uint8)
    assert lib.sb_render(eng._h, ctypes.byref(o), small.ctypes.data_as(ctypes.c_void_p), small.nbytes) == 1
    assert lib.sb_render(eng._h, None, np.zeros(512 * 512 * 3, np.uint8).ctypes.data_as(ctypes.c_void_p), 512 * 512 * 3) == 0
    eng.destroy()
    # ghost zones configured: not composited
    eng = sb.Engine(layout=2, max_particles=256, max_beams=512, collision_mode=OFF, path=TILED)
    eng.write_buffers(buf)
    eng.halo_configure([0, 1], [2, 3])
    with pytest.raises(EngineError) as ex:
        eng.render(64)
    assert ex.value.status == 6
    eng.destroy()


def test_determinism_and_device_output(sb):
    import torch
    buf = sb.scenes.default_buffers(1, 256, 512)
    eng = engine(sb, buf)
    eng.frame()
    a = eng.render(640)
    b = eng.render(640)
    assert np.array_equal(a, b)
    t = torch.full((640, 640, 3), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.render_device(t, 640)
    eng.sync()
    assert np.array_equal(t.cpu().numpy(), a)
    eng.destroy()


@pytest.mark.parametrize("mode,path", [(GRID, 0), (OFF, TILED)])
def test_no_side_effects(sb, mode, path):
    """frame, render, frame == frame, frame, bit for bit."""
    first = breaking_lattice(sb)
    out = []
    for render in (False, True):
        eng = engine(sb, first, 4000.0, collision_mode=mode, path=path)
        eng.frame()
        if render:
            eng.render(512)
            eng.render(2048)
        eng.frame()
        out.append(eng.load_buffers(first.copy()))
        eng.destroy()
    assert_same(out[1], out[0], "frame, render, frame")
