"""examples/c_abi_batch_raycast.c: sb_batch_raycast_device from plain C99 -- it builds everywhere and fails loudly without a GPU; on
the GPU the distances it prints for its fan of sixteen rays are, bit for bit, BatchEngine.raycast()'s for the same scene and rows."""
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
    exe = str(tmp_path / "c_abi_batch_raycast")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "c_abi_batch_raycast.c"), "-o", exe, "-L" + CSRC, "-lsoftbody_hip", "-Wl,-rpath," + CSRC,
                        "-lm", "-ldl"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_c_batch_raycast_example_builds_and_fails_loudly_without_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return  # (the GPU test below runs it)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_c_batch_raycast_example_runs(sb, tmp_path):
    import torch
    exe = build_example(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "C_ABI_BATCH_RAYCAST_OK" in p.stdout, p.stdout + p.stderr
    printed = re.findall(r"scene (\d) ray +(\d+): distance \S+ \(bits ([0-9a-f]{8})\) to (\w+) (-?\d+)", p.stdout)
    assert len(printed) == 2 * RAYS, p.stdout
    # the same scene and the same rows through the binding (the example computes its directions in double and rounds once)
    buf = sb.scenes.default_buffers(1, 128, 320)
    be = sb.BatchEngine(n_scenes=2, layout=1, max_particles=128, max_beams=320)
    be.write_scene(buf)
    turn = [2.0 * 3.14159265358979323846 * j / RAYS for j in range(RAYS)]
    direction = torch.tensor([[math.cos(a), math.sin(a)] for a in turn], dtype=torch.float64).to(torch.float32).cuda().expand(2, RAYS, 2)
    origin = torch.tensor([500.0, 300.0], device="cuda").expand(2, RAYS, 2).contiguous()
    mask = torch.tensor([[7], [5]], device="cuda").expand(2, RAYS)
    got = be.raycast(sb.batch.ray_rows(origin, direction, float("inf"), mask=mask))
    t, hit = got.t.cpu().numpy().view(np.uint32), got.hit.cpu().numpy()
    kinds = {"particle": 1, "beam": 2, "wall": 3}
    for s, j, bits, kind, index in printed:
        s, j = int(s), int(j)
        assert (int(bits, 16), kinds[kind], int(index)) == (int(t[s, j]), hit[s, j, 0], hit[s, j, 1]), (s, j, p.stdout)
    counts = got.counts.cpu().numpy()
    for s in range(2):
        assert "scene %d counts: valid %d, particles %d, beams %d, walls %d" % (s, *counts[s]) in p.stdout, p.stdout
    be.destroy()
