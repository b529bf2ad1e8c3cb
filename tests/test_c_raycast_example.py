"""examples/c_abi_raycast.c: sb_raycast from plain C99 -- it builds everywhere and fails loudly without a GPU; on the GPU the distances
it prints for its two fans of sixteen rays are, bit for bit, Engine.raycast()'s for the same scene and rows."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbody-webgpu_amd", "csrc")
RAYS = 16


def build_example(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    exe = str(tmp_path / "c_abi_raycast")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "c_abi_raycast.c"), "-o", exe, "-L" + CSRC, "-lsoftbody_hip", "-Wl,-rpath," + CSRC,
                        "-lm", "-ldl"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_c_raycast_example_builds_and_fails_loudly_without_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return  # (the GPU test below runs it)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_c_raycast_example_runs(sb, tmp_path):
    import torch
    exe = build_example(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "C_ABI_RAYCAST_OK" in p.stdout, p.stdout + p.stderr
    printed = re.findall(r"fan (\d) ray +(\d+): distance \S+ \(bits ([0-9a-f]{8})\) to (\w+) (-?\d+)", p.stdout)
    assert len(printed) == 2 * RAYS, p.stdout
    # the same scene and the same rows through the binding (the example computes its directions in double and rounds once)
    buf = sb.scenes.default_buffers(2, 128, 320)
    eng = sb.Engine(layout=2, max_particles=128, max_beams=320, collision_mode=0)
    eng.write_buffers(buf)
    turn = [2.0 * 3.14159265358979323846 * j / RAYS for j in range(RAYS)] * 2
    direction = torch.tensor([[math.cos(a), math.sin(a)] for a in turn], dtype=torch.float64).to(torch.float32).cuda()
    origin = torch.tensor([500.0, 300.0], device="cuda").expand(2 * RAYS, 2).contiguous()
    mask = torch.tensor([7] * RAYS + [5] * RAYS, device="cuda")
    got = eng.raycast(sb.engine.ray_rows(origin, direction, float("inf"), mask=mask))
    t, hit = got.t.cpu().numpy().view(np.uint32), got.hit.cpu().numpy()
    kinds = {"particle": 1, "beam": 2, "wall": 3}
    for f, j, bits, kind, index in printed:
        k = int(f) * RAYS + int(j)
        assert (int(bits, 16), kinds[kind], int(index)) == (int(t[k]), hit[k, 0], hit[k, 1]), (k, p.stdout)
    c = got.counts.cpu().numpy()
    assert "counts: valid %d, particles %d, beams %d, walls %d, swept %d, outside %d, long %d" % tuple(c[:7]) in p.stdout, p.stdout
    assert c[2] > 0, "the first fan meets beams"
    eng.destroy()
