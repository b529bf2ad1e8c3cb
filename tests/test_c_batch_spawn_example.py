"""examples/c_abi_batch_spawn.c: sb_batch_add_particles_device, sb_batch_add_beams_device and sb_batch_bodies_device from plain C99 -- it
builds everywhere and fails loudly without a GPU; on the GPU a spawned triangle leaves scene 0 of two default scenes with one body
more after a frame and scene 1 as it was."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbody-webgpu_amd", "csrc")


def build_example(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    exe = str(tmp_path / "c_abi_batch_spawn")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "c_abi_batch_spawn.c"), "-o", exe, "-L" + CSRC, "-lsoftbody_hip", "-Wl,-rpath," + CSRC,
                        "-lm", "-ldl"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_c_batch_spawn_example_builds_and_fails_loudly_without_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return  # (the GPU test below runs it)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_c_batch_spawn_example_runs(tmp_path):
    exe = build_example(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "C_ABI_BATCH_SPAWN_OK" in p.stdout, p.stdout + p.stderr
    assert "scene 0: bodies before 9, after 10; particles 119 120 121 (added 3, invalid 0, blocked 0, full 0); beams 299 300 301 (added 3)" in p.stdout, p.stdout
    assert "scene 1: bodies before 9, after 9; particles -1 -1 -1 (added 0, invalid 0, blocked 0, full 0); beams -1 -1 -1 (added 0)" in p.stdout, p.stdout
