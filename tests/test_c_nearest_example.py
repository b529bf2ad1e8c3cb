"""examples/c_abi_nearest.c: sb_nearest from plain C99 -- it builds everywhere and fails loudly without a GPU; on the GPU what it prints
for its two passes of sixteen points is, bit for bit, Engine.nearest()'s for the same scene and rows."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbody-webgpu_amd", "csrc")
POINTS = 16


def build_example(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    exe = str(tmp_path / "c_abi_nearest")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "c_abi_nearest.c"), "-o", exe, "-L" + CSRC, "-lsoftbody_hip", "-Wl,-rpath," + CSRC,
                        "-lm", "-ldl"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_c_nearest_example_builds_and_fails_loudly_without_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return  # (the GPU test below runs it)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_c_nearest_example_runs(sb, tmp_path):
    import torch
    exe = build_example(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "C_ABI_NEAREST_OK" in p.stdout, p.stdout + p.stderr
    printed = re.findall(r"pass (\d) point +(\d+): distance \S+ \(bits ([0-9a-f]{8})\) to (\w+) (-?\d+) at .*? within reach (\d+) particles (\d+) beams", p.stdout)
    assert len(printed) == 2 * POINTS, p.stdout
    # the same scene and the same rows through the binding
    buf = sb.scenes.default_buffers(2, 128, 320)
    eng = sb.Engine(layout=2, max_particles=128, max_beams=320, collision_mode=0)
    eng.write_buffers(buf)
    j = torch.arange(2 * POINTS, device="cuda") % POINTS
    pts = torch.stack((15.0 + 62.5 * j.float(), 75.0 + 20.0 * j.float()), 1)
    rmax = torch.tensor([60.0] * POINTS + [float("inf")] * POINTS, device="cuda")
    mask = torch.tensor([7] * POINTS + [1] * POINTS, device="cuda")
    got = eng.nearest(sb.batch.point_rows(pts[None], rmax, mask=mask)[0])
    d, hit, within = got.d.cpu().numpy().view(np.uint32), got.hit.cpu().numpy(), got.within.cpu().numpy()
    kinds = {"nothing": 0, "particle": 1, "beam": 2, "wall": 3}
    for f, i, bits, kind, index, in_p, in_b in printed:
        k = int(f) * POINTS + int(i)
        assert (int(bits, 16), kinds[kind], int(index), int(in_p), int(in_b)) == (int(d[k]), hit[k, 0], hit[k, 1], within[k, 0], within[k, 1]), (k, p.stdout)
    c = got.counts.cpu().numpy()
    assert "counts: valid %d, particles %d, beams %d, walls %d, swept %d, outside %d, long %d" % tuple(c[:7]) in p.stdout, p.stdout
    assert c[2] > 0, "the first pass finds beams"
    eng.destroy()
