"""examples/c_abi_batch_render.c: plain C99 -> sb_batch (4 default scenes, one frame) -> sb_batch_render_scene of scene 0 -> a PPM
file, equal to host/render.js's picture (tests/render_ref.py) of the state one frame of the default scene leaves in the oracle."""
import os
import subprocess

import numpy as np
import pytest

from render_ref import ppm, render_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbody-webgpu_amd", "csrc")


def build(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    exe = str(tmp_path / "c_abi_batch_render")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "c_abi_batch_render.c"), "-o", exe, "-lm", "-L" + CSRC, "-lsoftbody_hip",
                        "-Wl,-rpath," + CSRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_c_batch_render_example_builds(tmp_path):
    assert os.path.exists(build(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("res", [64, 301])
def test_c_batch_render_example_picture(sb, oracle, tmp_path, res):
    exe = build(tmp_path)
    out = tmp_path / "scene0.ppm"
    p = subprocess.run([exe, str(out), str(res)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "C_BATCH_RENDER_OK 4 scenes of 119 particles, 299 beams" in p.stdout, p.stdout + p.stderr
    buf = sb.scenes.default_buffers(1, 256, 512)
    ref = oracle.OracleEngine(1000.0, 10.0, 64, 1, oracle.COLLIDE_ALLPAIRS)
    ref.write_buffers(buf)
    ref.frame()
    want = ppm(render_ref(ref.load_buffers(buf.copy()), res, 1000.0, 10.0))
    got = out.read_bytes()
    assert len(got) == len(want)
    assert got == want, "%d bytes differ" % int((np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8)).sum())
