"""tests/batch_raycast_ref.py, the numpy restatement of sb_batch_raycast_device: hand-built scenes on integer
coordinates whose t is known exactly; ties; row codes; csrc/sb_batch_ray_math.h on the host (tests/batch_ray_check.cpp,
`make hostcheck`) against the restatement bit for bit on the whole case set; two wrong models are caught; the binding's names."""
import os
import subprocess

import numpy as np
import pytest

import batch_raycast_cases as cases
import batch_raycast_ref as ref
from test_hostcheck_cpu import CSRC, ENV

F = np.float32


@pytest.fixture(scope="module")
def case_set(sb):
    return cases.case_set(sb)


def by_name(case_set, name):
    return next(c for c in case_set if c["name"] == name)


def check_expect(c):
    """both modes of a hand-built scene: every row with a stated answer gives exactly it"""
    seen = 0
    for labels, expect in ((None, c["expect"]), (c["labels"], c["expect_labelled"])):
        t, hit, counts = ref.raycast_ref(c["buf"], c["rows"], cases.BOUNDS, cases.RADIUS, labels)
        for j, (want_t, kind, index) in expect.items():
            assert (int(t[j]), hit[j, 0], hit[j, 1]) == (int(F(want_t).view(np.uint32)), kind, index), (c["name"], labels is not None, j, t.view(F)[j], hit[j])
            seen += 1
        assert counts[0] == (hit[:, 0] >= 0).sum() and counts[1:].tolist() == [(hit[:, 0] == k).sum() for k in (1, 2, 3)]
    return seen


def test_exact_integer_cases(case_set):
    """1: discs (t = 90, 45 with D = (2, 0), 0 inside, a ray that stops short, a zero D), beams (t = 60, parallel, both endpoints
    touched exactly, den < 0), the four walls from the centre"""
    assert check_expect(by_name(case_set, "discs and walls")) == 24 and check_expect(by_name(case_set, "beams")) == 14
    c = by_name(case_set, "discs and walls")
    t, hit, counts = ref.raycast_ref(c["buf"], c["rows"])
    assert t.view(F)[[0, 1, 2, 3]].tolist() == [90.0, 45.0, 0.0, 89.0] and hit[6:10, 1].tolist() == [1, 2, 4, 8]
    assert t.view(F)[6:10].tolist() == [500.0] * 4 and counts.tolist() == [12, 5, 0, 5]
    assert hit[:, 2].tolist() == [-1] * cases.K, "no labels: every label word is -1"


def test_ties(case_set):
    """2: the same t bits: the smaller data index, then particle before beam; a skipped label lets the ray past"""
    c = by_name(case_set, "ties")
    assert check_expect(c) == 10
    tied = []
    t, hit, _ = ref.raycast_ref(c["buf"], c["rows"], labels=c["labels"], ties=tied)
    assert tied[:3] == [2, 2, 1] and hit[:5, 2].tolist() == [2, 7, 7, -1, 5], "the labels of the hits: the beam's is its endpoint A's"


def test_row_codes(case_set):
    """3: empty, every cause of invalid, -0 in t becomes +0, tmax bits verbatim on a miss"""
    c = by_name(case_set, "row codes")
    assert check_expect(c) == 28
    t, hit, counts = ref.raycast_ref(c["buf"], c["rows"])
    assert hit[:14, 0].tolist() == [-1] + [-2] * 10 + [0, -1, 1] and counts.tolist() == [2, 1, 0, 0] and not t[:11].any()
    assert (hit[14:, 0] == -1).all(), "the padding rows are empty rows"
    d = by_name(case_set, "discs and walls")
    assert ref.raycast_ref(d["buf"], d["rows"])[0][11] == 0, "+0, not -0"


def test_coverage(case_set):
    """4a: the set exercises every kind, both row codes, exact ties and skipped labels"""
    cov = cases.coverage(case_set)
    print(cov)
    assert cov["kinds"] == {ref.MISS, ref.PARTICLE, ref.BEAM, ref.WALL, ref.EMPTY, ref.INVALID}
    assert cov["tie_rows"] >= 1 and cov["skips"] >= 3
    per_case = [set(ref.raycast_ref(c["buf"], c["rows"], labels=c["labels"])[1][:, 0].tolist()) for c in case_set]
    assert all({1, 2, 3} <= k for c, k in zip(case_set, per_case) if c["name"] in ("default", "sparse permuted mapping", "full capacity"))
    assert per_case[9] <= {0, 3, -1}, "never uploaded: walls only"


def records(case_set, labelled):
    """the file tests/batch_ray_check.cpp reads, and the lines it must print"""
    words, lines = [], []
    for c in case_set:
        labels = c["labels"] if labelled else None
        g = ref.geometry(c["buf"], labels)
        head = np.array([g.pidx.size, g.bidx.size, len(c["rows"]), int(labelled)], np.uint32)
        u = lambda x: np.asarray(x, F).view(np.uint32)
        part = np.stack([g.pidx.astype(np.uint32), u(g.px), u(g.py), g.plab.astype(np.int32).view(np.uint32)], 1)
        beam = np.stack([g.bidx.astype(np.uint32), u(g.ax), u(g.ay), u(g.bx), u(g.by), g.blab.astype(np.int32).view(np.uint32)], 1)
        words += [head, u([cases.BOUNDS, cases.RADIUS]), part.ravel(), beam.ravel(), c["rows"].ravel()]
        t, hit, _ = ref.raycast_ref(c["buf"], c["rows"], cases.BOUNDS, cases.RADIUS, labels)
        lines += ["%08x %d %d" % (int(t[j]), hit[j, 0], hit[j, 1]) for j in range(len(t))]
    return np.concatenate(words).astype("<u4").tobytes(), lines


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_header_against_restatement_under_sanitizers(case_set, san, tmp_path):
    """4b: csrc/sb_batch_ray_math.h, as a program of its own, prints the restatement's t bits, kinds and indices for every row of
    the twelve scenes, without and with labels"""
    target = os.path.join("hostcheck_build", "batch_ray_check_" + san)
    p = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    for labelled in (False, True):
        data, want = records(case_set, labelled)
        path = tmp_path / ("rays_%d.bin" % labelled)
        path.write_bytes(data)
        p = subprocess.run([os.path.join(CSRC, target), str(path)], capture_output=True, text=True, timeout=300, env=ENV)
        assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
        got = p.stdout.split("\n")
        assert got[len(want)] == "BATCH_RAY_CHECK_OK 12 %d" % (12 * cases.K), got[-3:]
        bad = [(i // cases.K, i % cases.K, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, bad[:10]


def test_wrong_models_are_caught(case_set):
    """5: "the first meeting in slot order" and "a pending beam does not count" both differ from the definition on the set"""
    first = drop = 0
    for c in case_set:
        want = ref.raycast_ref(c["buf"], c["rows"], labels=c["labels"])
        a = ref.raycast_ref(c["buf"], c["rows"], labels=c["labels"], model="first")
        b = ref.raycast_ref(c["buf"], c["rows"], labels=c["labels"], drop=c["pending"])
        first += int((a[0] != want[0]).sum())
        drop += int((b[0] != want[0]).sum() + (b[1] != want[1]).any(axis=1).sum())
    c = by_name(case_set, "removed and pending beams")
    _, hit, _ = ref.raycast_ref(c["buf"], c["rows"])
    assert set(hit[:5, 1].tolist()) <= set(c["pending"]) and (hit[:5, 0] == ref.BEAM).all(), "rows 0 .. 4 meet a pending beam first"
    assert not set(hit[:, 1][hit[:, 0] == ref.BEAM].tolist()) & set(c["removed"]), "a removed beam is met by nothing"
    assert first >= 10 and drop >= 5, (first, drop)


def test_binding_names(sb):
    b = sb.batch
    assert b.RAY_HIT_FIELDS == ref.HIT_FIELDS and len(b.RAY_HIT_FIELDS) == b.RAY_HIT_WORDS == ref.HIT_WORDS
    assert b.RAY_COUNT_FIELDS == ref.COUNT_FIELDS and len(b.RAY_COUNT_FIELDS) == b.RAY_COUNT_WORDS == ref.COUNT_WORDS
    assert (b.RAY_PARTICLES, b.RAY_BEAMS, b.RAY_WALLS, b.RAY_MAX, b.RAY_ROW_WORDS) == (ref.PARTICLES, ref.BEAMS, ref.WALLS, ref.RAY_MAX, ref.ROW_WORDS)
    assert (b.RAY_MISS, b.RAY_PARTICLE, b.RAY_BEAM, b.RAY_WALL, b.RAY_EMPTY, b.RAY_INVALID) == (0, 1, 2, 3, -1, -2)
    assert (b.WALL_LEFT, b.WALL_RIGHT, b.WALL_LOW, b.WALL_HIGH) == (ref.WALL_LEFT, ref.WALL_RIGHT, ref.WALL_LOW, ref.WALL_HIGH)
    assert b.RayCast._fields == ref.RayCast._fields and sb.RAY_HIT_FIELDS == b.RAY_HIT_FIELDS and sb.RAY_COUNT_FIELDS == b.RAY_COUNT_FIELDS
    assert "sb_batch_raycast_device" in sb.engine.declared_symbols()
