"""tests/batch_nearest_ref.py, the numpy restatement of sb_batch_nearest_device: hand-built scenes on integer
coordinates whose answers are known exactly; ties; the radius boundary; row codes; `within`; non-finite positions; pending and
removed beams; csrc/sb_batch_near_math.h on the host (tests/batch_near_check.cpp, `make hostcheck`) against the restatement bit for
bit on the whole case set; two wrong models are caught; the binding's names and the header's constants."""
import os
import re
import subprocess

import numpy as np
import pytest

import batch_nearest_cases as cases
import batch_nearest_ref as ref
from test_hostcheck_cpu import CSRC, ENV

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda x: int(F(x).view(np.uint32))


@pytest.fixture(scope="module")
def case_set(sb):
    return cases.case_set(sb)


def by_name(case_set, name):
    return next(c for c in case_set if c["name"] == name)


def check_expect(c):
    """both modes of a hand-built scene: every row with a stated answer gives exactly it"""
    seen = 0
    for labels, expect, within in ((None, c["expect"], c["expect_within"]), (c["labels"], c["expect_labelled"], {**c["expect_within"], **c["expect_within_labelled"]})):
        d, hit, point, win, counts = ref.nearest_ref(c["buf"], c["rows"], cases.BOUNDS, labels)
        for j, (want_d, kind, index, qx, qy) in expect.items():
            got = (int(d[j]), hit[j, 0], hit[j, 1], int(point[j, 0]), int(point[j, 1]))
            assert got == (bits(want_d), kind, index, bits(qx), bits(qy)), (c["name"], labels is not None, j, d.view(F)[j], hit[j], point.view(F)[j])
            seen += 1
        for j, want in within.items():
            if labels is None and ref.verdict(c["rows"][j], False) != ref.MISS:
                want = (0, 0)
            assert tuple(win[j]) == want, (c["name"], labels is not None, j, win[j])
        assert counts[0] == (hit[:, 0] >= 0).sum() and counts[1:].tolist() == [(hit[:, 0] == k).sum() for k in (1, 2, 3)]
        assert not win[hit[:, 0] < 0].any() and not d[hit[:, 0] < 0].any() and not point[hit[:, 0] < 0].any(), "empty and invalid rows give zeros"
    return seen


def test_exact_integer_cases(case_set):
    """1: the segment (0, 0) -> (4, 0) from (1, 3): u = 0.25, Q = (1, 0), d = 3; both clamps; d = +0 on a particle; a degenerate
    beam answers as its endpoint A; the four walls; the radius boundary: rmax = 3 keeps d2 = 9, the float below 3 gives a miss that
    returns its own bits, rmax = 0 keeps only d2 = 0"""
    c = by_name(case_set, "segments")
    assert check_expect(c) == 30
    d, hit, point, win, counts = ref.nearest_ref(c["buf"], c["rows"])
    assert d.view(F)[:5].tolist() == [3.0, 2.0, 5.0, 0.0, 3.0] and d[3] == 0, "+0 on a particle"
    assert d[6] == bits(cases.BELOW_3) and d[6] == bits(3.0) - 1 and hit[6].tolist() == [0, -1, -1] and hit[5].tolist() == [2, 0, -1]
    assert hit[:, 2].tolist() == [-1] * cases.K, "no labels: every label word is -1"
    assert counts.tolist() == [15, 3, 6, 4]


def test_ties(case_set):
    """2: equal d2 bits: the smaller data index; a particle before the beam clamped to it; a beam before a wall; the smaller wall
    word; a skipped label lets the answer pass to the next"""
    c = by_name(case_set, "ties")
    assert check_expect(c) == 16
    tied = []
    _, hit, _, _, _ = ref.nearest_ref(c["buf"], c["rows"], labels=c["labels"], ties=tied)
    assert tied[:4] == [2, 2, 1, 2] and tied[6] == 2 and hit[:8, 2].tolist() == [2, 7, 7, 7, -1, 5, -1, 7], "the labels: a beam's is its endpoint A's"


def test_row_codes(case_set):
    """3: empty, the five causes of invalid, rmax = -0, a miss returns rmax's bits and the query point"""
    c = by_name(case_set, "row codes")
    assert check_expect(c) == 30
    d, hit, point, _, counts = ref.nearest_ref(c["buf"], c["rows"])
    assert hit[:15, 0].tolist() == [-1] + [-2] * 10 + [1, -1, 1, 0] and counts.tolist() == [3, 2, 0, 0] and not d[:11].any()
    assert (hit[15:, 0] == -1).all(), "the padding rows are empty rows"
    assert point[14].tolist() == [bits(150), bits(80)] and d[14] == bits(20)


def test_within_masks_and_non_finite(case_set):
    """4: `within` with each mask bit off and under skip_label; a NaN position is never kept, an infinite one only under rmax = +inf"""
    assert check_expect(by_name(case_set, "masks and within")) == 0
    assert check_expect(by_name(case_set, "non-finite positions")) == 10


def test_coverage(case_set):
    """5: the set exercises every kind, both row codes, the three branches of the segment test, exact ties and skipped labels"""
    cov = cases.coverage(case_set)
    print(cov)
    assert cov["kinds"] == {ref.MISS, ref.PARTICLE, ref.BEAM, ref.WALL, ref.EMPTY, ref.INVALID}
    assert cov["branches"] == {ref.AT_A, ref.AT_B, ref.INSIDE}
    assert cov["tie_rows"] >= 5 and cov["skips"] >= 3
    per_case = [set(ref.nearest_ref(c["buf"], c["rows"], labels=c["labels"])[1][:, 0].tolist()) for c in case_set]
    assert all({1, 2, 3} <= k for c, k in zip(case_set, per_case) if c["name"] in ("default", "sparse permuted mapping", "full capacity"))
    assert case_set[cases.NEVER_UPLOADED]["buf"] is None and per_case[cases.NEVER_UPLOADED] <= {0, 3, -1}, "never uploaded: walls only"


def records(case_set, labelled):
    """the file tests/batch_near_check.cpp reads, and the lines it must print"""
    words, lines = [], []
    for c in case_set:
        labels = c["labels"] if labelled else None
        g = ref.geometry(c["buf"], labels)
        head = np.array([g.pidx.size, g.bidx.size, len(c["rows"]), int(labelled)], np.uint32)
        u = lambda x: np.asarray(x, F).view(np.uint32)
        part = np.stack([g.pidx.astype(np.uint32), u(g.px), u(g.py), g.plab.astype(np.int32).view(np.uint32)], 1)
        beam = np.stack([g.bidx.astype(np.uint32), u(g.ax), u(g.ay), u(g.bx), u(g.by), g.blab.astype(np.int32).view(np.uint32)], 1)
        words += [head, u([cases.BOUNDS]), part.ravel(), beam.ravel(), c["rows"].ravel()]
        d2 = []
        _, hit, point, win, _ = ref.nearest_ref(c["buf"], c["rows"], cases.BOUNDS, labels, d2_bits=d2)
        won = hit[:, 0] > 0
        lines += ["%08x %d %d %08x %08x %d %d" % (d2[j], hit[j, 0], hit[j, 1], point[j, 0] if won[j] else 0, point[j, 1] if won[j] else 0, win[j, 0], win[j, 1])
                  for j in range(len(hit))]
    return np.concatenate(words).astype("<u4").tobytes(), lines


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_header_against_restatement_under_sanitizers(case_set, san, tmp_path):
    """6: csrc/sb_batch_near_math.h, as a program of its own, prints the restatement's d2 bits, kinds, indices, closest points and
    `within` for every row of the twelve scenes, without and with labels"""
    target = os.path.join("hostcheck_build", "batch_near_check_" + san)
    p = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    for labelled in (False, True):
        data, want = records(case_set, labelled)
        path = tmp_path / ("points_%d.bin" % labelled)
        path.write_bytes(data)
        p = subprocess.run([os.path.join(CSRC, target), str(path)], capture_output=True, text=True, timeout=300, env=ENV)
        assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
        got = p.stdout.split("\n")
        assert got[len(want)] == "BATCH_NEAR_CHECK_OK 12 %d" % (12 * cases.K), got[-3:]
        bad = [(i // cases.K, i % cases.K, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, bad[:10]


def test_wrong_models_are_caught(case_set):
    """7: "the first kept primitive in slot order" and "a pending beam does not count" both differ from the definition on the set;
    a removed beam is nobody's nearest"""
    first = drop = 0
    for c in case_set:
        want = ref.nearest_ref(c["buf"], c["rows"], labels=c["labels"])
        a = ref.nearest_ref(c["buf"], c["rows"], labels=c["labels"], model="first")
        b = ref.nearest_ref(c["buf"], c["rows"], labels=c["labels"], drop=c["pending"])
        first += int((a[0] != want[0]).sum())
        drop += int(((b[0] != want[0]) | (b[1] != want[1]).any(axis=1) | (b[3] != want[3]).any(axis=1)).sum())
    c = by_name(case_set, "removed and pending beams")
    _, hit, _, win, _ = ref.nearest_ref(c["buf"], c["rows"])
    assert (win[:5, 1] >= 1).all() and (hit[:5, 0] == ref.BEAM).all(), "rows 0 .. 4 have a pending beam within reach"
    dropped = ref.nearest_ref(c["buf"], c["rows"], drop=c["pending"])
    assert (dropped[3][:5, 1] == win[:5, 1] - 1).all(), "each of them counts"
    assert not set(hit[:, 1][hit[:, 0] == ref.BEAM].tolist()) & set(c["removed"]), "a removed beam is nearest to nothing"
    assert first >= 10 and drop >= 5, (first, drop)


def test_binding_names_and_abi(sb):
    b = sb.batch
    assert b.NEAR_HIT_FIELDS == ref.HIT_FIELDS and len(b.NEAR_HIT_FIELDS) == b.NEAR_HIT_WORDS == ref.HIT_WORDS
    assert b.NEAR_COUNT_FIELDS == ref.COUNT_FIELDS and len(b.NEAR_COUNT_FIELDS) == b.NEAR_COUNT_WORDS == ref.COUNT_WORDS
    assert b.NEAR_WITHIN_FIELDS == ref.WITHIN_FIELDS
    assert b.Nearest._fields == ref.Nearest._fields and sb.NEAR_HIT_FIELDS == b.NEAR_HIT_FIELDS and sb.NEAR_COUNT_FIELDS == b.NEAR_COUNT_FIELDS
    assert sb.point_rows is b.point_rows
    assert "sb_batch_nearest_device" in sb.engine.declared_symbols()
    # the header's constants are batch.py's
    header = open(os.path.join(ROOT, "include", "softbody.h")).read()
    define = lambda name: int(re.search(r"#define %s \(?(-?\d+)u?\)?" % name, header).group(1))
    assert (define("SB_BATCH_NEAR_MAX"), define("SB_NEAR_PARTICLES"), define("SB_NEAR_BEAMS"), define("SB_NEAR_WALLS")) == \
        (b.NEAR_MAX, b.NEAR_PARTICLES, b.NEAR_BEAMS, b.NEAR_WALLS) == (ref.NEAR_MAX, ref.PARTICLES, ref.BEAMS, ref.WALLS)
    assert (define("SB_BATCH_NEAR_HIT_WORDS"), define("SB_BATCH_NEAR_COUNT_WORDS")) == (b.NEAR_HIT_WORDS, b.NEAR_COUNT_WORDS)
    assert [define("SB_BATCH_NEAR_" + n) for n in ("MISS", "PARTICLE", "BEAM", "WALL", "EMPTY", "INVALID")] == \
        [b.NEAR_MISS, b.NEAR_PARTICLE, b.NEAR_BEAM, b.NEAR_WALL, b.NEAR_EMPTY, b.NEAR_INVALID] == [0, 1, 2, 3, -1, -2]
    assert define("SB_ABI_VERSION") == 1 and b.NEAR_ROW_WORDS == ref.ROW_WORDS == 8


def test_abi_in_c(sb, tmp_path):
    """sizeof(sb_batch_near_point) == 32 and SB_ABI_VERSION == 1, asked of a C compiler; sb_abi_version() == 1 of the built library"""
    src = tmp_path / "abi.c"
    src.write_text('#include "softbody.h"\n_Static_assert(sizeof(sb_batch_near_point) == 32, "row");\n_Static_assert(SB_ABI_VERSION == 1, "abi");\n'
                   '_Static_assert(SB_BATCH_NEAR_MAX == 256, "max");\nint main(void) { return 0; }\n')
    p = subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "abi")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    import __graft_entry__ as ge
    ge.build()
    assert sb.engine.load_library().sb_abi_version() == 1
