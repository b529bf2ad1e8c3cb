"""The engine's ray casts on the CPU (sb_raycast_device): tests/raycast_ref.py -- brute force with the wide key -- gives
the batch restatement's t / hit and words 0 .. 3 on every scene of the batch's case set; the rules behind the cost words; and
csrc/sb_ray_walk.h as a program of its own (tests/ray_walk_check.cpp, `make hostcheck`) under ASan + UBSan and TSan: the walk leaves
out nothing the float tests would meet, and two wrong walks are caught on named cases."""
import os
import subprocess

import numpy as np
import pytest

import batch_raycast_cases as cases
import batch_raycast_ref as bref
import raycast_ref as ref
from test_hostcheck_cpu import CSRC, ENV

F = np.float32


def test_wide_key_restatement_equals_the_batch_restatement(sb):
    for c in cases.case_set(sb):
        for labels in (None, c["labels"]):
            t, hit, counts = bref.raycast_ref(c["buf"], c["rows"], cases.BOUNDS, cases.RADIUS, labels)
            got = ref.raycast_ref(c["buf"], c["rows"], cases.BOUNDS, cases.RADIUS, labels)
            assert np.array_equal(got.t, t) and np.array_equal(got.hit, hit) and got.counts[:4].tolist() == counts.tolist(), c["name"]
            assert got.counts[7] == 0 and got.counts.dtype == np.int64


def test_wide_key_orders_as_the_definition():
    t = np.array([1.0, 1.0, 1.0, 0.5], F)
    k = [ref.wide_keys(t[i:i + 1], F(ref.INF), kind, index)[0] for i, (kind, index) in enumerate(((2, 5), (1, 2 ** 30 - 1), (1, 70000), (3, 8)))]
    assert k[3] < k[2] < k[1] < k[0] < ref.NO_KEY
    assert ref.wide_keys(np.array([-0.0], F), F(0.0), 3, 1)[0] == np.uint64(3 << 30 | 1), "-0 becomes +0"


def test_cell_rule_classification_and_gate(sb):
    assert [ref.default_cap(p) for p in (0, 1, 7, 8, 17, 18, 2 * 8192 ** 2 + 5)] == [1, 1, 1, 2, 2, 3, 8192]
    assert ref.grid(2048, 4000.0, 10.0) == (32, F(125.0)) and ref.grid(10 ** 6, 1000.0, 10.0)[0] == 49, "reduced until the cell is 2r(1 + 1/64) wide"
    assert ref.grid(100, 1000.0, 10.0, cells_per_side=3) == (3, F(1000.0) / F(3.0)) and ref.grid(100, 1000.0, 1e-9) == (1, F(1000.0))
    assert ref.coord(np.array([-1.0, 0.0, 99.9, 100.0, 1000.0, np.nan], F), 100.0, 10).tolist() == [0, 0, 0, 1, 9, 0]
    assert ref.in_grid(np.array([0.0, 1000.0, 1000.1, np.inf, np.nan], F), np.zeros(5, F), 1000.0).tolist() == [True, True, False, False, False]
    c = next(c for c in cases.case_set(sb) if c["name"] == "NaN and infinite coordinates")
    g = ref.geometry(c["buf"])
    G, cell = ref.grid(g.pidx.size, cases.BOUNDS, cases.RADIUS)
    outside, long_beams = ref.leftovers(g, cases.BOUNDS, G, cell)
    assert outside == 4 and long_beams >= 4, "the four particles made NaN or infinite, and every beam at them"
    assert ref.leftovers(g, cases.BOUNDS, 1, F(1000.0))[1] == long_beams, "one cell: only beams with an end outside are long"
    row = lambda *r: bref.pack([r])[0]
    B = cases.BOUNDS
    assert ref.walkable(row(7, -B, 2 * B, 1, 0, 5), B) and not ref.walkable(row(7, -B - 0.5, 0, 1, 0, 5), B) and not ref.walkable(row(7, 0, 2 * B + 0.5, 1, 0, 5), B)
    assert not ref.walkable(row(7, 0, 0, 0, 0, 5), B) and ref.walkable(row(7, 0, 0, 2.0 ** -20, 0, 5), B) and not ref.walkable(row(7, 0, 0, 2.0 ** -21, 0, 5), B)
    assert ref.walkable(row(7, 0, 0, 2.0 ** 20, 0, 5), B) and not ref.walkable(row(7, 0, 0, 2.0 ** 20, 2.0 ** 10, 5), B)


@pytest.fixture(scope="module")
def programs():
    out = {}
    for san in ("asan", "tsan"):
        target = os.path.join("hostcheck_build", "ray_walk_check_" + san)
        p = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        out[san] = os.path.join(CSRC, target)
    return out


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=ENV)


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_walk_header_under_sanitizers(programs, san):
    """(a) and (b) on the drawn scene at cells_per_side 1, 2, 3, 64 and the default rule; the program asserts its own coverage:
    hits whose centre is farther than r from the line in double (the slack at work), tangents from beyond 2 bounds, early exits,
    rows the leftover list wins, rows the gate refuses"""
    p = run(programs[san])
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
    words = p.stdout.split()
    assert words[0] == "RAY_WALK_CHECK_OK", p.stdout
    stat = dict(zip(words[1::2], words[2::2]))
    print(stat)
    assert int(stat["slack_hits"]) >= 1 and int(stat["far_tangents"]) >= 1 and int(stat["exits"]) >= 50 and int(stat["default_G"]) == 33


def test_wrong_walks_are_caught(programs):
    """the walk without its pad loses the disc one row up; at the exact exit bound `<=` in place of `<` loses the tie of two discs in
    different columns; the right walk passes both named cases"""
    exe = programs["asan"]
    for case in ("pad", "tie"):
        p = run(exe, "0", case)
        assert p.returncode == 0 and "RAY_WALK_CHECK_OK" in p.stdout, (case, p.stdout, p.stderr)
    p = run(exe, "1", "pad")
    assert p.returncode == 1 and "LOST (a) pad" in p.stderr and "LOST (b) pad" in p.stderr, (p.stdout, p.stderr)
    p = run(exe, "2", "tie")
    assert p.returncode == 1 and "LOST (b) tie of two discs" in p.stderr and p.stderr.count("LOST") == 1, (p.stdout, p.stderr)
    assert "0000000040000007, brute force" in p.stderr.replace("42b40000", "00000000"), "the later column's smaller index was not seen"


def test_binding_names(sb):
    e = sb.engine
    assert e.RAYCAST_COUNT_FIELDS == ref.COUNT_FIELDS and len(e.RAYCAST_COUNT_FIELDS) == e.RAYCAST_COUNT_WORDS == ref.COUNT_WORDS
    assert e.RayCast._fields == ref.RayCast._fields and ctypes_size(e) == 32
    assert {"sb_raycast_device", "sb_raycast"} <= set(e.declared_symbols())


def ctypes_size(e):
    import ctypes
    return ctypes.sizeof(e.SbRaycastOptions)
