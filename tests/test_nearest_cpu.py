"""The engine's proximity queries on the CPU (sb_nearest_device): tests/nearest_ref.py -- brute force with the wide key
-- gives the batch restatement's d / hit / point / within and words 0 .. 3 on every scene of the batch's case set; the key's order;
the gate and ring rules behind word 4 on hand-made rows; and csrc/sb_near_walk.h as a program of its own (tests/near_walk_check.cpp,
`make hostcheck`) under ASan + UBSan and TSan: the rings leave out nothing that is kept or could win, and three wrong walks are
caught on named cases."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import batch_nearest_cases as cases
import batch_nearest_ref as bref
import nearest_ref as ref
from test_hostcheck_cpu import CSRC, ENV

F = np.float32
INF = ref.INF


def test_wide_key_restatement_equals_the_batch_restatement(sb):
    for c in cases.case_set(sb):
        if c["buf"] is None:   # never uploaded: an engine has no such state
            continue
        for labels in (None, c["labels"]):
            d, hit, point, within, counts = bref.nearest_ref(c["buf"], c["rows"], cases.BOUNDS, labels)
            got = ref.nearest_ref(c["buf"], c["rows"], cases.BOUNDS, 10.0, labels)
            assert ref.same(got, ref.Nearest(d, hit, point, within, got.counts)) == [], c["name"]
            assert got.counts[:4].tolist() == counts.tolist() and got.counts[7] == 0 and got.counts.dtype == np.int64, c["name"]


def test_wide_key_orders_as_the_definition(sb):
    d2 = np.array([4.0, 4.0, 4.0, 1.0], F)
    k = [ref.wide_keys(d2[i:i + 1], F(INF), kind, index)[0] for i, (kind, index) in enumerate(((2, 5), (1, 2 ** 30 - 1), (1, 70000), (3, 8)))]
    assert k[3] < k[2] < k[1] < k[0] < ref.NO_KEY, "index 2^30 - 1 fits below the kind"
    assert ref.wide_keys(np.array([9.0], F), F(8.99), 1, 0)[0] == ref.NO_KEY and ref.wide_keys(np.array([9.0], F), F(9.0), 1, 0)[0] != ref.NO_KEY
    # a particle beats the beam that ends in it: the 'ties' scene, row 1
    c = next(c for c in cases.case_set(sb) if c["name"] == "ties")
    got = ref.nearest_ref(c["buf"], c["rows"], cases.BOUNDS, 10.0)
    assert got.hit[1].tolist()[:2] == [1, 9] and got.hit[2].tolist()[:2] == [2, 3]


def test_gate_and_ring_rules():
    B = 1000.0
    row = lambda *r: bref.pack([r])[0]
    assert ref.local(row(7, -B, 2 * B, INF), B) and not ref.local(row(7, -B - 0.5, 0, INF), B) and not ref.local(row(7, 0, 2 * B + 0.5, INF), B)
    assert ref.ring_of(np.array([-3, -2, -1, 0, 1, 2])).tolist() == [2, 1, 0, 0, 1, 2], "one more column towards lower x"
    assert ref.bound2(0, 100.0, B) == -1.0 and ref.bound2(1, 100.0, B) == ((100.0 - B * 2.0 ** -20) * (1.0 - 2.0 ** -20)) ** 2
    G, cell = 10, F(100.0)
    none = np.zeros(0, np.uint64)
    cells = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    need = lambda r, keys=none, rc=cells, within=True, wall=ref.NO_KEY, **kw: ref.rings_needed(r, keys, wall, rc, B, G, cell, within, **kw)
    assert need(row(4, 550, 550, INF)) == 0, "walls only: nothing to look for"
    assert need(row(7, 550, 550, 0)) == 2, "rmax 0: ring 0 has no bound, ring 1 has"
    assert need(row(7, 550, 550, 99.9)) == 2 and need(row(7, 550, 550, 100)) == 3, "rmax against (100 - 2^-20 bounds)(1 - 2^-20)"
    assert need(row(7, 550, 550, INF)) == 5, "rmax inf with within: until the rings cover the grid -- rings 0 .. 4 from cell 5 of 10"
    assert need(row(7, 550, 550, INF), max_rings=4) is None and need(row(7, 550, 550, INF), max_rings=5) == 5
    assert need(row(7, -950, 550, 10), max_rings=1) == 1, "the rings outside the grid cost nothing: cx = -10 starts at ring 10, whose bound ends it"
    assert need(row(7, -950, 550, INF), max_rings=9) is None and need(row(7, -950, 550, INF), max_rings=10) == 10, "rings 10 .. 19 cover the grid"
    key = ref.wide_keys(np.array([50.0 ** 2], F), F(INF), 1, 0)
    assert need(row(1, 550, 550, INF), key, (np.array([5]), np.array([5])), within=False) == 2, "without within it stops at the winner"
    assert need(row(1, 550, 550, INF), key, (np.array([5]), np.array([5])), within=True) == 5
    far = ref.wide_keys(np.array([240.0 ** 2], F), F(INF), 1, 0)
    assert need(row(1, 550, 550, INF), far, (np.array([7]), np.array([5])), within=False) == 4, "seen in ring 2; 240 is below L(3), not below L(2)"
    assert need(row(5, 550, 20, INF), none, cells, within=False, wall=ref.wide_keys(np.array([400.0], F), F(INF), 3, 4)[0]) == 2, "a wall can end the walk"


@pytest.fixture(scope="module")
def programs():
    out = {}
    for san in ("asan", "tsan"):
        target = os.path.join("hostcheck_build", "near_walk_check_" + san)
        p = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        out[san] = os.path.join(CSRC, target)
    return out


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=900, env=ENV)


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_walk_header_under_sanitizers(programs, san):
    """the drawn scene at cells_per_side 1, 2, 3, 64 and the default rule, max_rings 1, 2 and the default, with and without within;
    the program asserts its own coverage.  The thresholds above 1 are a third of what the right walk shows (stopped 17670, covered 7123,
    out_of_rings 11399, outside_gate 210, leftover_wins 137, low_beam_wins 54, slack_beams 2732)."""
    p = run(programs[san])
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
    words = p.stdout.split("NEAR_WALK_CHECK_OK", 1)[1].split()
    stat = dict(zip(words[0::2], words[1::2]))
    print(stat)
    assert int(stat["default_G"]) == 33
    for name, least in (("stopped", 5000), ("covered", 2000), ("out_of_rings", 3000), ("outside_gate", 70), ("leftover_wins", 40), ("low_beam_wins", 15),
                        ("slack_beams", 900)):
        assert int(stat[name]) >= least, (name, stat)


def test_wrong_walks_are_caught(programs):
    """no extra cell loses the beam recorded one column left; `<=` at the exact bound loses the tie of two particles in different
    rings; no 2^-20 bounds term loses the particle that coord() rounds into the next cell; the right walk passes all three"""
    exe = programs["asan"]
    for case in ("low", "tie", "slack"):
        p = run(exe, "0", case)
        assert p.returncode == 0 and "NEAR_WALK_CHECK_OK" in p.stdout, (case, p.stdout, p.stderr)
    for model, case, lost in (("1", "low", "LOST low"), ("2", "tie", "LOST tie of two particles"), ("3", "slack", "LOST slack")):
        p = run(exe, model, case)
        assert p.returncode == 1 and lost in p.stderr and p.stderr.count("LOST") == 1, (model, case, p.stdout, p.stderr)
    assert "4880000040000007, brute force 4880000040000003" in run(exe, "2", "tie").stderr, "the farther ring's smaller index was not seen"


def test_binding_names(sb):
    e = sb.engine
    assert e.NEAREST_COUNT_FIELDS == ref.COUNT_FIELDS and len(e.NEAREST_COUNT_FIELDS) == e.NEAREST_COUNT_WORDS == ref.COUNT_WORDS
    assert e.Nearest._fields == ref.Nearest._fields and ctypes.sizeof(e.SbNearestOptions) == 32
    assert {"sb_nearest_device", "sb_nearest"} <= set(e.declared_symbols())
