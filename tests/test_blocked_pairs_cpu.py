"""What the beam phase of the blocked kernel evaluates against what its substeps need, replayed from the plan on the CPU
(tools/blocked_prefix_waste.cpp, plain g++): with entry slots paired up over neighbouring entries every entry inside a
substep's prefix is evaluated exactly once per substep, and no thread group holds more than one entry past the prefix."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("prefix_waste") / "blocked_prefix_waste")
    p = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "softbody-webgpu_amd", "csrc"),
                        os.path.join(ROOT, "tools", "blocked_prefix_waste.cpp"), "-o", out], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return out


def test_paired_slots_cover_every_prefix_once_on_a_70x70_plan(exe):
    p = subprocess.run([exe, "70", "70", "256", "7", "1", "2", "3", "6", "7"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "PREFIX_WASTE_OK" in p.stdout, p.stdout + p.stderr
    rows = re.findall(r"^(strided|paired)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+[\d.]+\s+(\d+)\s+(\d+)\s+(\d+)$", p.stdout, re.M)
    assert len(rows) == 10, p.stdout
    for name, evaluated, needed, past, padding, groups_run, _, _ in rows:
        evaluated, needed, past, padding, groups_run = int(evaluated), int(needed), int(past), int(padding), int(groups_run)
        assert evaluated == needed + past + padding == 2 * groups_run        # every needed entry once, the rest past or padding
        if name == "paired":
            assert past + padding <= groups_run                               # at most one of a group's two
    by = {}
    for name, evaluated, *_ in rows:
        by.setdefault(name, []).append(int(evaluated))
    assert all(p_ <= s_ for p_, s_ in zip(by["paired"], by["strided"]))
