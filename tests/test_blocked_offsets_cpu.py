"""The byte offsets of the blocked kernel's range-checked loads and stores (csrc/sb_blocked_addr.h) on the CPU with a plain g++
build: for randomly drawn tile tables -- the counts at 0, 1, the slot boundaries and capacity, tiles that end their arrays, arrays
just short of 4 GiB -- every in-range slot's offset is size * (base + j) and inside the descriptor, every out-of-range slot's offset
is at or past the descriptor's size (tests/blocked_offsets_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blocked_offsets(tmp_path):
    out = str(tmp_path / "blocked_offsets_check")
    p = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "softbody-webgpu_amd", "csrc"),
                        os.path.join(ROOT, "tests", "blocked_offsets_check.cpp"), "-o", out], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "BLOCKED_OFFSETS_OK" in p.stdout, p.stdout + p.stderr
