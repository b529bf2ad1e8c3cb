"""examples/c_abi_batch_pose.c: sb_batch_pose_device from plain C99 -- it builds everywhere and fails loudly without a GPU; on the GPU
what it prints for its lattice turned by a quarter turn is BatchEngine.pose()'s for the same scene."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbody-webgpu_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_example(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    exe = str(tmp_path / "c_abi_batch_pose")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "c_abi_batch_pose.c"), "-o", exe, "-L" + CSRC, "-lsoftbody_hip", "-Wl,-rpath," + CSRC,
                        "-lm", "-ldl"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_c_batch_pose_example_builds_and_fails_loudly_without_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return  # (the GPU test below runs it)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_c_batch_pose_example_runs(sb, tmp_path):
    import torch
    import batch_pose_cases as pc
    exe = build_example(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "C_ABI_BATCH_POSE_OK" in p.stdout, p.stdout + p.stderr
    printed = re.search(r"a (\S+), b (\S+), I (\S+)", p.stdout)
    assert printed, p.stdout
    # the same scene through the binding (layout 1, identity mapping)
    i = np.arange(9)
    lattice = np.stack([100.0 + 10.0 * (i % 3), 200.0 + 10.0 * (i // 3)], axis=1).astype("f4")
    turned = np.stack([110.0 - (lattice[:, 1] - 210.0) + 50.0, 210.0 + (lattice[:, 0] - 110.0) - 20.0], axis=1).astype("f4")
    be = sb.BatchEngine(n_scenes=1, layout=1, max_particles=16, max_beams=8)
    be.write_scene(pc.scene_of(sb, lattice, None, (16, 8), layout=1))
    state = torch.zeros((1, 16, 6), dtype=torch.float32, device="cuda")
    state[0, :9, 0:2] = torch.from_numpy(turned).cuda()
    be.write_particles_device(state)
    labels = torch.full((1, 16), -1, dtype=torch.int32, device="cuda")
    labels[0, :9] = 0
    got = be.pose(labels, rows=1, moments=True)
    assert [float(x) for x in printed.groups()] == got.moments[0, 0, :3].tolist() == [0.0, 1200.0, 1200.0], p.stdout
    assert "particles 9, label 0, matched 9, unmatched 0" in p.stdout
    assert "centroid %.9g %.9g, reference centroid %.9g %.9g" % tuple(got.rows[0, 0, 4:8].tolist()) in p.stdout
    be.destroy()
