"""sb_batch_body_summary_device without a GPU: declared, exported, bound with its prototype, every argument error before a device
is looked for; tests/batch_body_summary_ref.py on a scene worked out by hand in which the tree order shows; a sequential replay of
the kernel's sparse route, equal by bits to the dense masked trees; the one-body identity with the scene summary; and the oracle
side of every program of tests/test_gpu_batch_body_summary.py, with the figures the GPU test relies on."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_bodies_ref as br  # noqa: E402
import batch_body_summary_cases as qc  # noqa: E402
import batch_body_summary_ref as qr  # noqa: E402
import batch_summary_cases as sc  # noqa: E402
import batch_summary_ref as sr  # noqa: E402


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_header_declares_and_library_exports_the_call(sb):
    names = sb.engine.declared_symbols()
    L = sb.batch.load_library()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert "sb_batch_body_summary_device" in names and hasattr(L, "sb_batch_body_summary_device")
    assert L.sb_batch_body_summary_device.restype is ctypes.c_int
    assert L.sb_batch_body_summary_device.argtypes == [vp, vp, u32, vp, vp]
    assert L.sb_abi_version() == 1   # additions only
    header = open(sb.engine.HEADER_PATH).read()
    for needle in ("#define SB_BATCH_BODY_SUMMARY_WORDS 24u", "body_summary_words", "body_summary_kernel_vgprs",
                   "body_summary_kernel_scratch_bytes", "body_summary_lds_bytes", "still writes +0.0"):
        assert needle in header, needle
    assert callable(sb.BatchEngine.body_summary)


def test_fields_name_the_24_words(sb):
    f, s = sb.batch.BODY_SUMMARY_FIELDS, sb.batch.SUMMARY_FIELDS
    assert sb.batch.BODY_SUMMARY_WORDS == qr.WORDS == 24 == len(f) == len(set(f))
    assert [f[w] for w in qr.SUMMARY_SHARED_WORDS] == [s[w] for w in qr.SUMMARY_SHARED_WORDS]   # the same word, the same name
    assert f[2] == "label" and f[19] == "angular_momentum" and f[20:] == ("reserved_20", "reserved_21", "reserved_22", "reserved_23")
    assert sorted(qr.COUNT_WORDS + qr.SUM_WORDS + qr.EXTREME_WORDS) == list(range(24))


def test_every_argument_error_comes_before_a_device(sb):
    L = sb.batch.load_library()
    word = (ctypes.c_int32 * 64)()
    p = ctypes.cast(word, ctypes.c_void_p)
    for args in ((None, None, 0, None, None), (None, p, 1, p, p), (None, p, 0, p, None)):
        assert L.sb_batch_body_summary_device(*args) == 1
    assert b"sb_batch_body_summary_device" in L.sb_batch_last_error(None)


def test_python_refuses_what_is_not_a_buffer_or_a_row_count(sb):
    be = sb.BatchEngine.__new__(sb.BatchEngine)
    be._h, be.device, be.n_scenes, be.max_particles, be.max_beams, be._ext_stream = None, 0, 2, 16, 16, None
    import torch
    labels = torch.zeros((2, 16), dtype=torch.int32)   # (on the CPU: refused like everything else here)
    for call in (lambda: be.body_summary("no"), lambda: be.body_summary(labels), lambda: be.body_summary(rows=0),
                 lambda: be.body_summary(rows=17), lambda: be.body_summary(rows=2.0), lambda: be.body_summary(rows=True),
                 lambda: be.body_summary(out=torch.zeros((2, 8, 24), dtype=torch.float32)), lambda: be.body_summary(rank=1.5),
                 lambda: be.body_summary(rank=torch.zeros((2, 16), dtype=torch.int32))):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------- by hand
def hand_scene(sb):
    """Capacity 8 / 8 (W = 8).  Group 4 = data indices {0, 1, 4} with x = 2^60, 1, -2^60: the tree adds leaves 0 and 4 first
    (h = 4) and gives 1; a sum in index order gives 2^60 + 1 = 2^60, then 0.  Group 2 = {2, 3, 5, 6}, interleaved with group 4 in
    index space: 2 and 6 meet at h = 4, 3 at h = 1 only, 5 joins 4's subtree -- where group 4's leaf is masked.  Data index 7
    is labelled -1.  Beams (data index: a - b)  0: 0 - 1,  1: 1 - 4,  2: 2 - 3,  3: 4 - 5 (across groups),  4: 6 - 7 (7 in no group)."""
    buf = sb.Buffers(2, 8, 8)
    pts = np.zeros((8, 6), "f4")
    pts[:, 0] = [2.0 ** 60, 1.0, 3.0, 2.0 ** -30, -2.0 ** 60, 2.0 ** 30, 5.0, 100.0]
    pts[:, 1] = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    pts[:, 2] = [1.0, -1.0, 0.5, 0.0, 2.0, 0.0, -0.5, 9.0]
    pts[:, 3] = [0.0, 1.0, 0.0, 3.0, 0.0, 0.0, 0.25, 9.0]
    beams = np.zeros(5, sb.layout.BEAM_DTYPE[2])
    for k, (a, b) in enumerate([(0, 1), (1, 4), (2, 3), (4, 5), (6, 7)]):
        beams[k]["a"], beams[k]["b"], beams[k]["length"] = a, b, 10.0
        beams[k]["strain"], beams[k]["stress"] = 0.125 * (k + 1), -1.0 * k
    buf.set_scene(pts, beams)
    return buf, np.array([4, 4, 2, 2, 4, 2, 2, -1], np.int32)


def test_reference_on_a_scene_worked_out_by_hand(sb):
    buf, labels = hand_scene(sb)
    rows, rank = qr.body_summary_ref(buf, labels, 3, pending_slots=np.array([0, 1, 1, 1, 1, 0, 0, 0], bool))
    assert rank.tolist() == [1, 1, 0, 0, 1, 0, 0, -1]                      # 4 particles before 3
    a, b = rows[1], rows[0]
    assert a[:6].tolist() == [3, 2, 4, 1, 0, 0] and b[:6].tolist() == [4, 1, 2, 1, 0, 0]   # beams 3 and 4 belong to no group
    assert a[6] == np.float32(1.0 / 3.0) and a[6] != 0.0                   # the tree's order, not the index order
    serial = np.float64(0.0)
    for x in buf.particles[[0, 1, 4], 0]:
        serial = serial + np.float64(x)
    assert serial == 0.0
    # group 2 in the tree: h = 4 adds leaf 6 onto leaf 2 (3 + 5) and leaf 5 onto the masked leaf 1 (0 + 2^30); h = 2 adds s[2] onto the
    # masked s[0] and leaf 3 onto s[1] (2^30 + 2^-30 rounds to 2^30); h = 1 adds the two
    tree = (np.float64(0.0) + (np.float64(3.0) + np.float64(5.0))) + ((np.float64(0.0) + np.float64(2.0 ** 30)) + np.float64(2.0 ** -30))
    assert tree == 2.0 ** 30 + 8.0 and b[6] == np.float32(tree / 4.0)
    assert a[7] == np.float32(8.0 / 3.0) and a[10:14].tolist() == [-2.0 ** 60, 1.0, 2.0 ** 60, 5.0]
    assert a[14] == np.float32(0.5 + 1.0 + 2.0) and a[15] == 4.0
    assert a[19] == np.float32(-1.0 + 3.0 - 10.0)                          # x vy - y vx: (0 - 1), (1 + 2), (0 - 10)
    assert a[16:19].tolist() == [0.25, 0.0, -1.0] and b[16:19].tolist() == [0.375, -2.0, -2.0]
    assert not a[20:].any() and not b[20:].any()
    assert bits(rows[2]).tolist() == bits(qr.empty_row()).tolist() and rows[2][2] == -1
    one, rank1 = qr.body_summary_ref(buf, labels, 1)
    assert bits(one[0]).tolist()[:3] == bits(b).tolist()[:3] and one[0][3] == 0 and rank1.tolist() == rank.tolist()   # cut, still ranked
    none = qr.body_summary_ref(buf, np.full(8, 8, np.int32), 2)
    assert (none[1] == -1).all() and bits(none[0]).tolist() == [bits(qr.empty_row()).tolist()] * 2
    assert [x.tolist() for x in map(bits, qr.never_uploaded(8, 2))] == [bits(none[0]).tolist(), bits(none[1]).tolist()]


# ---------------------------------------------------------------- the kernel's route against the dense trees
def dense_sums(grp, member, leaves, W):
    out = {}
    for g in sorted(set(int(x) for x in grp[member])):
        leaf = np.zeros(W, np.float64)
        sel = member & (grp == g)
        leaf[np.nonzero(sel)[0]] = leaves[sel]
        out[g] = sr.tree_sum(leaf) + 0.0
    return out


@pytest.mark.parametrize("W", [8, 128, 1024])
def test_the_sparse_route_gives_the_bits_of_the_masked_trees(W):
    rng = np.random.default_rng(W)
    maxP = W if W != 128 else 65      # (a capacity that is no power of two: leaves 65 .. 127 are never members)
    i = np.arange(maxP)
    groupings = {"random few": rng.integers(0, 3, maxP), "random many": rng.integers(0, maxP, maxP), "singles": i.copy(),
                 "all in one": np.full(maxP, maxP - 1), "interleaved": i % 2,
                 "out of range": np.where(rng.random(maxP) < 0.3, rng.choice([-1, maxP, qr.INT32_MIN], maxP), rng.integers(0, 4, maxP))}
    for name, grp in groupings.items():
        grp = grp.astype(np.int64)
        member = (grp >= 0) & (grp < maxP) & (rng.random(maxP) < (1.0 if name == "all in one" else 0.9))
        for scale in (1.0, 2.0 ** 40):   # wide magnitudes: nearly every addition rounds, so another order gives other bits
            leaves = (rng.standard_normal(maxP) * scale ** rng.random(maxP)).astype(np.float32).astype(np.float64)
            leaves[rng.random(maxP) < 0.05] = -0.0
            got, exp = replay_route(grp, member, leaves, W), dense_sums(grp, member, leaves, W)
            assert sorted(got) == sorted(exp), name
            for g in exp:
                assert np.float64(got[g]).view(np.uint64) == np.float64(exp[g]).view(np.uint64), (W, name, g, got[g], exp[g])
    if W == 1024:   # and the order does matter: a sum in index order differs somewhere
        grp, member = np.zeros(maxP, np.int64), np.ones(maxP, bool)
        leaves = (rng.standard_normal(maxP) * (2.0 ** 40) ** rng.random(maxP)).astype(np.float32).astype(np.float64)
        serial = np.float64(0.0)
        for x in leaves:
            serial = serial + x
        assert replay_route(grp, member, leaves, W)[0] == dense_sums(grp, member, leaves, W)[0] != serial


replay_route = qr.replay_route


def test_a_group_of_all_leaves_of_minus_zero_is_the_one_exception():
    W = 8
    leaves = np.full(W, -0.0)
    assert np.signbit(sr.tree_sum(leaves)) and not np.signbit(sr.tree_sum(leaves) + 0.0)
    assert not np.signbit(replay_route(np.zeros(W, np.int64), np.ones(W, bool), leaves, W)[0])
    leaves[3] = 0.0   # any +0.0, or any absent leaf, and the tree itself gives +0.0
    assert not np.signbit(sr.tree_sum(leaves))


# ---------------------------------------------------------------- the programs of the GPU tests, on the oracle
@pytest.fixture(scope="module")
def expected(sb, oracle):
    """Every stepped case on the oracle, once: {name: (case, {op index: (bufs_now, labels, pending)}, oracles)}."""
    out = {}
    for case in qc.stepped_cases(sb):
        exp, refs = qc.expected(oracle, case)
        out[case["name"]] = (case, exp, refs)
    return out


def rows_of(exp_k, max_rows, labels=None):
    now, body_labels, pending = exp_k
    return qr.body_summary_of(now, body_labels if labels is None else labels, max_rows, pending)


def test_one_body_rows_equal_the_scene_summary_by_bits(expected):
    case, exp, refs = expected["yield / break / delete"]
    seen = 0
    for k in case["compare_after"]:
        now, labels, pending = exp[k]
        rows, rank = rows_of(exp[k], 2)
        for i, (buf, up) in enumerate(zip(now, case["bufs"])):
            if len(set(labels[i][labels[i] >= 0].tolist())) != 1:
                continue
            srow = sr.summary_ref(buf, up, int(pending[i].sum()))
            w = list(qr.SUMMARY_SHARED_WORDS)
            sr.assert_rows_equal(np.where(np.isin(np.arange(24), w), rows[i, 0], srow), srow, "scene %d after op %d" % (i, k))
            assert rows[i, 0, 2] == 0 and bits(rows[i, 1]).tolist() == bits(qr.empty_row()).tolist()
            assert (rank[i][labels[i] >= 0] == 0).all()
            seen += 1
    assert seen == 4   # scenes 0 and 5, after the frames and mid-frame


def test_every_program_runs_on_the_oracle_and_the_rows_add_up(expected):
    assert len(expected) == 5
    with np.errstate(all="raise"):   # (the finite cases raise no warning in the reference)
        for name, (case, exp, refs) in expected.items():
            if name == "force saturation":
                continue
            maxP = case["cap"][0]
            for k in case["compare_after"]:
                now, labels, pending = exp[k]
                rows, rank = rows_of(exp[k], maxP)
                for i, buf in enumerate(now):
                    P = 0 if buf is None else buf.particle_count
                    Bc = 0 if buf is None else buf.beam_count
                    assert rows[i, :, 0].sum() == P and rows[i, :, 1].sum() == Bc, (name, k, i)
                    assert (rank[i] >= 0).sum() == P and (np.diff(rows[i, :, 0]) <= 0).all(), (name, k, i)
                    n = int((rows[i, :, 2] >= 0).sum())
                    assert n == br.bodies_ref(buf)[2][0] if buf is not None else n == 0, (name, k, i)
                    assert rows[i, :, 3].sum() == (0 if buf is None else int(pending[i][:Bc].sum())), (name, k, i)


def test_the_recorded_figures(expected):
    case, exp, refs = expected["default scene at 120 / 300"]
    rows, rank = rows_of(exp[0], 8)
    assert case["program"] == [("frame", 2)] and rows[0, :, 0].tolist() == [40, 36, 25, 4, 4, 4, 4, 1]   # 9 bodies: the last is cut
    assert rank[0].max() == 8 and (rank[0] == 8).sum() == 1 and np.isfinite(rows[0, :7]).all() and np.isnan(rows[0, 7, 16:19]).all()
    case, exp, refs = expected["yield / break / delete"]
    rows, rank = rows_of(exp[0], 4)
    assert [int((rank[i].max()) + 1) for i in range(6)] == [1, 6, 21, 38, 56, 1] and rows[:, 0, 0].tolist() == [144, 139, 120, 101, 84, 144]
    mid = rows_of(exp[1], 4)[0]
    assert mid[:, :, 3].sum() > 0 and rows[:, :, 3].sum() == 0
    case, exp, refs = expected["heterogeneous"]
    grabbed, deleted = (rows_of(exp[k], 4)[0] for k in case["compare_after"])
    assert grabbed[qc.LATTICE, 0, :4].tolist() == [144, grabbed[qc.LATTICE, 0, 1], 0, 129] and grabbed[qc.LATTICE, 1, 2] == -1
    assert grabbed[2, 0, 3] == 220 and deleted[qc.LATTICE, :, 0].tolist() == [110, 19, 3, 3] and deleted[:, :, 3].sum() == 0
    assert deleted[2, 0, 0] == 967 and bits(deleted[4]).tolist() == bits(deleted[5]).tolist() == [bits(qr.empty_row()).tolist()] * 4
    case, exp, refs = expected["permuted mapping + coincident particles"]
    rows, rank = rows_of(exp[case["compare_after"][0]], 8)
    assert (rank[0, :50] == -1).all() and rows[0, 0, 0] == 40 and rows[0, 0, 2] >= 50 and rows[1, :, 0].tolist()[:6] == [2, 1, 1, 1, 1, 0]


def test_callers_labels_and_non_finite_particles_on_the_oracle(expected):
    case, exp, refs = expected["yield / break / delete"]
    now, body_labels, pending = exp[0]
    n, maxP = len(now), case["cap"][0]
    L = qc.caller_labels(n, maxP)
    rows, rank = rows_of(exp[0], 4, L["stripes"])
    assert rows[0, :3, 2].tolist() == [0, 1, 2] and rows[0, :3, 0].sum() == 144 and rows[0, 3, 2] == -1
    assert 0 < rows[0, :, 1].sum() < now[0].beam_count                    # beams across two stripes belong to none
    for name in ("none", "too large", "INT32_MIN"):
        rows, rank = rows_of(exp[0], 2, L[name])
        assert (rank == -1).all() and bits(rows).tolist() == bits(np.broadcast_to(qr.empty_row(), rows.shape)).tolist(), name
    rows, rank = rows_of(exp[0], 2, L["split"])
    assert set(rows[0, :, 2].tolist()) == {2, 5} and rows[0, :, 0].sum() == 144
    rows, rank = rows_of(exp[0], 3, L["mixed"])
    assert rows[0, :, 2].tolist() == [0, 1, -1] and (rank[0] == -1).sum() >= maxP // 2
    case, exp, refs = expected["force saturation"]
    k = case["compare_after"][0]
    now = exp[k][0]
    N = qc.nonfinite_labels(len(now))
    rows, rank = rows_of(exp[k], 2, N["one group"])
    bad = rows[sc.NONFINITE_SCENE]
    assert bad[0, :6].tolist() == [6, 3, 0, 0, 2, 1] and np.isfinite(bad[0, 6:20]).all() and bad[1, 2] == -1
    rows, rank = rows_of(exp[k], 2, N["non-finite apart"])
    bad = rows[sc.NONFINITE_SCENE]
    assert bad[:, 0].tolist() == [4, 2] and bad[1, 2] == 3 and bad[1, 4] == 2                 # the count is kept
    assert np.isnan(bad[1, 6:14]).all() and np.isnan(bad[1, 15]) and bad[1, 14] == 0 == bad[1, 19] and bad[1, 1] == 0
    assert rows[0, :, :6].tolist() == [[1, 0, 0, 0, 0, 0], [1, 0, 3, 0, 0, 0]]                 # a finite scene beside it: its beam is cut in two


def test_the_graphs_are_ranked_as_they_are_called(sb):
    for case in qc.graph_cases(sb):
        maxP = case["cap"][0]
        labels = qr.body_labels_of(case["bufs"], maxP)
        rows, rank = qr.body_summary_of(case["bufs"], labels, maxP)
        assert [int((r[:, 2] >= 0).sum()) for r in rows] == case["groups"], case["name"]
        for i, buf in enumerate(case["bufs"]):
            if buf is not None and buf.particle_count:
                assert rows[i, :, 0].sum() == buf.particle_count and rows[i, :, 1].sum() == buf.beam_count, (case["name"], i)
                assert np.isfinite(rows[i, 0]).all(), (case["name"], i)
                assert buf.particle_count == 2 or (rows[i, 0, 8] != 0 and rows[i, 0, 19] != 0), (case["name"], i)   # (the random velocities)
    case = qc.case_limit(sb)
    rows, rank = qr.body_summary_of(case["bufs"], qr.body_labels_of(case["bufs"], 1024), 16)
    pieces = rows[1]
    assert (pieces[:, 0] == 64).all() and (np.diff(pieces[:, 2]) > 0).all() and pieces[0, 2] == 0   # the tie: labels ascending
    assert rows[0, 0, 0] == 1024 and rows[2, :, 0].tolist() == [2] * 16 and (rank[2] >= 16).sum() == 1024 - 32
    assert [c["cap"] for c in qc.graph_cases(sb)] == [(1024, 4096), (8, 8), (65, 64)]
