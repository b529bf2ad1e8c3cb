"""The entry-word codec and LDS plane offsets of the blocked kernel (csrc/sb_blocked_word.h) on the CPU with a plain g++ build:
repack and unpack over region indices at every edge of the fields and all 16 narrow rows, the wide form for rows a narrow word
cannot name, dead entries, and the planes (tests/blocked_word_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blocked_word_codec(tmp_path):
    out = str(tmp_path / "blocked_word_check")
    p = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "softbody-webgpu_amd", "csrc"),
                        os.path.join(ROOT, "tests", "blocked_word_check.cpp"), "-o", out], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "BLOCKED_WORD_OK" in p.stdout, p.stdout + p.stderr
