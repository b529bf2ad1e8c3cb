"""examples/c_abi_batch_nearest.c: sb_batch_nearest_device from plain C99 -- it builds everywhere and fails loudly without a GPU; on
the GPU what it prints for its grid of sixteen probe points is, bit for bit, BatchEngine.nearest()'s for the same scene and rows."""
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
    exe = str(tmp_path / "c_abi_batch_nearest")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "c_abi_batch_nearest.c"), "-o", exe, "-L" + CSRC, "-lsoftbody_hip", "-Wl,-rpath," + CSRC,
                        "-lm", "-ldl"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_c_batch_nearest_example_builds_and_fails_loudly_without_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return  # (the GPU test below runs it)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_c_batch_nearest_example_runs(sb, tmp_path):
    import torch
    exe = build_example(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "C_ABI_BATCH_NEAREST_OK" in p.stdout, p.stdout + p.stderr
    printed = re.findall(r"scene (\d) point +(\d+): distance \S+ \(bits ([0-9a-f]{8})\) to (\w+) (-?\d+) at \((\S+), (\S+)\), within: (\d+) particles, (\d+) beams", p.stdout)
    assert len(printed) == 2 * POINTS, p.stdout
    # the same scene and the same rows through the binding
    buf = sb.scenes.default_buffers(1, 128, 320)
    be = sb.BatchEngine(n_scenes=2, layout=1, max_particles=128, max_beams=320)
    be.write_scene(buf)
    j = torch.arange(POINTS, device="cuda")
    point = torch.stack([100.0 + 250.0 * (j % 4).float(), 50.0 + 150.0 * (j // 4).float()], dim=1).expand(2, POINTS, 2).contiguous()
    mask = torch.tensor([[7], [5]], device="cuda").expand(2, POINTS)
    got = be.nearest(sb.batch.point_rows(point, 120.0, mask=mask))
    d, hit, q, within = got.d.cpu().numpy().view(np.uint32), got.hit.cpu().numpy(), got.point.cpu().numpy(), got.within.cpu().numpy()
    kinds = {"nothing": 0, "particle": 1, "beam": 2, "wall": 3}
    for s, j, bits, kind, index, qx, qy, n_p, n_b in printed:
        s, j = int(s), int(j)
        assert (int(bits, 16), kinds[kind], int(index)) == (int(d[s, j]), hit[s, j, 0], hit[s, j, 1]), (s, j, p.stdout)
        assert (np.float32(qx), np.float32(qy), int(n_p), int(n_b)) == (q[s, j, 0], q[s, j, 1], within[s, j, 0], within[s, j, 1]), (s, j, p.stdout)
    counts = got.counts.cpu().numpy()
    for s in range(2):
        assert "scene %d counts: valid %d, particles %d, beams %d, walls %d" % (s, *counts[s]) in p.stdout, p.stdout
    be.destroy()
