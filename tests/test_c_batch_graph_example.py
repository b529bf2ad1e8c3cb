"""examples/c_abi_batch_graph.c: sb_batch_graph_device from plain C99 -- it builds everywhere and fails loudly without a GPU; on the
GPU the counts of two default scenes, and after one weld of the two free particles one beam and two connected particles more in
scene 0, the new edge in `ends` and `nbr`, scene 1 as it was."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbody-webgpu_amd", "csrc")


def build_example(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    exe = str(tmp_path / "c_abi_batch_graph")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "c_abi_batch_graph.c"), "-o", exe, "-L" + CSRC, "-lsoftbody_hip", "-Wl,-rpath," + CSRC,
                        "-lm", "-ldl"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_c_batch_graph_example_builds_and_fails_loudly_without_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return  # (the GPU test below runs it)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_c_batch_graph_example_runs(tmp_path):
    exe = build_example(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "C_ABI_BATCH_GRAPH_OK" in p.stdout, p.stdout + p.stderr
    assert "scene 0 before: beams 299, connected particles 117, largest degree 8 at particle 13" in p.stdout, p.stdout
    assert "scene 0 after:  beams 300, connected particles 119, largest degree 8 at particle 13" in p.stdout, p.stdout
    assert "scene 1 after:  beams 299, connected particles 117, largest degree 8 at particle 13" in p.stdout, p.stdout
    assert "the weld: beam 299 joins {44, 45}" in p.stdout, p.stdout
