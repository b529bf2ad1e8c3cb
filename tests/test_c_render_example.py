"""examples/c_abi_render.c: plain C99 -> sb_render -> a PPM file, equal to host/render.js's picture (tests/render_ref.py) of the
state two frames of the default scene leave (the oracle's golden snapshot: the engine reproduces it bit for bit)."""
import os
import subprocess

import numpy as np
import pytest

from render_ref import ppm, render_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbody-webgpu_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def build(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    exe = str(tmp_path / "c_abi_render")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "c_abi_render.c"), "-o", exe, "-lm", "-L" + CSRC, "-lsoftbody_hip",
                        "-Wl,-rpath," + CSRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_c_render_example_builds(tmp_path):
    assert os.path.exists(build(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("res", [512, 301])
def test_c_render_example_picture(sb, tmp_path, res):
    exe = build(tmp_path)
    out = tmp_path / "frame.ppm"
    p = subprocess.run([exe, str(out), str(res)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "C_RENDER_OK 119 particles, 299 beams" in p.stdout, p.stdout + p.stderr
    gold = sb.scenes.default_buffers(1)   # (the v1 snapshot's size check wants room for twice the counts: engineMapping.ts:418)
    assert gold.load_snapshot(open(os.path.join(GOLDEN, "default_scene_v1_after_2_frames.snapshot"), "rb").read())
    want = ppm(render_ref(gold, res, 1000.0, 10.0))
    got = out.read_bytes()
    assert got == want, "%d bytes differ" % int((np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8)).sum())
