"""sb_batch_pose_device without a GPU: declared, exported, bound with its prototype, every argument error before a device is looked
for; tests/batch_pose_ref.py on scenes worked out by hand, where small-integer coordinates make everything exact; a sequential
replay of the kernel's sparse route, equal by bits to the dense masked trees; the identity with the body summary's means;
csrc/sb_batch_pose_math.h on the host under sanitizers (tests/batch_pose_check.cpp) against the restatement, bit for bit; the
geometric property's bounds on the restatement; and the oracle side of the programs of tests/test_gpu_batch_pose.py, with the
figures the GPU test relies on."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_body_summary_cases as qc  # noqa: E402
import batch_body_summary_ref as qr  # noqa: E402
import batch_pose_cases as pc  # noqa: E402
import batch_pose_ref as pr  # noqa: E402
from test_hostcheck_cpu import CSRC  # noqa: E402


def b32(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def b64(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_the_call(sb):
    names = sb.engine.declared_symbols()
    L = sb.batch.load_library()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert "sb_batch_pose_device" in names and hasattr(L, "sb_batch_pose_device")
    assert L.sb_batch_pose_device.restype is ctypes.c_int
    assert L.sb_batch_pose_device.argtypes == [vp, vp, vp, u32, vp, vp, vp]
    assert L.sb_abi_version() == 1   # additions only
    header = open(sb.engine.HEADER_PATH).read()
    for needle in ("#define SB_BATCH_POSE_WORDS 24u", "#define SB_BATCH_POSE_MOMENT_WORDS 8u", "pose_words", "pose_moment_words",
                   "pose_lds_bytes", "pose_kernel_vgprs", "pose_kernel_scratch_bytes", "0x7FF8000000000000"):
        assert needle in header, needle
    assert callable(sb.BatchEngine.pose) and callable(sb.batch.pose_fit) and sb.pose_fit is sb.batch.pose_fit


def test_fields_name_the_words(sb):
    f, m = sb.batch.POSE_FIELDS, sb.batch.POSE_MOMENT_FIELDS
    assert sb.batch.POSE_WORDS == pr.WORDS == 24 == len(f) == len(set(f))
    assert sb.batch.POSE_MOMENT_WORDS == pr.MOMENT_WORDS == 8 == len(m) == len(set(m))
    assert f[:4] == ("particles", "label", "matched", "unmatched") and f[10:17] == m[:5] + ("angular_velocity", "stretch_sq")
    assert m[5] == "matched" and f[4:6] == qr_fields(sb)[6:8] and f[8:10] == qr_fields(sb)[8:10]
    assert sb.POSE_FIELDS is f and sb.POSE_MOMENT_FIELDS is m


def qr_fields(sb):
    return sb.batch.BODY_SUMMARY_FIELDS


def test_every_argument_error_comes_before_a_device(sb):
    L = sb.batch.load_library()
    word = (ctypes.c_int64 * 64)()
    p = ctypes.cast(word, ctypes.c_void_p)
    for args in ((None, None, None, 0, None, None, None), (None, p, None, 1, p, p, p), (None, p, p, 0, p, None, None),
                 (None, None, None, 1, p, None, None), (None, p, None, 1, None, None, None)):
        assert L.sb_batch_pose_device(*args) == 1
    assert b"sb_batch_pose_device: null batch" in L.sb_batch_last_error(None)


def test_python_refuses_what_is_not_a_buffer_or_a_row_count(sb):
    be = sb.BatchEngine.__new__(sb.BatchEngine)
    be._h, be.device, be.n_scenes, be.max_particles, be.max_beams, be._ext_stream = None, 0, 2, 16, 16, None
    import torch
    labels = torch.zeros((2, 16), dtype=torch.int32)   # (on the CPU: refused like everything else here)
    for call in (lambda: be.pose("no"), lambda: be.pose(labels), lambda: be.pose(rows=0), lambda: be.pose(rows=17),
                 lambda: be.pose(rows=2.0), lambda: be.pose(rows=True), lambda: be.pose(out=torch.zeros((2, 8, 24), dtype=torch.float32)),
                 lambda: be.pose(rank=1.5), lambda: be.pose(moments=torch.zeros((2, 8, 8), dtype=torch.float64)),
                 lambda: be.pose(ref=torch.zeros((2, 16, 2), dtype=torch.float32)), lambda: be.pose(ref="no"),
                 lambda: sb.batch.pose_fit(torch.zeros((2, 8, 8), dtype=torch.float32)), lambda: sb.batch.pose_fit(torch.zeros((2, 7), dtype=torch.float64))):
        with pytest.raises(ValueError):
            call()


def test_pose_fit_is_the_documented_arithmetic(sb):
    import torch
    m = torch.tensor([[25.0, 25.0, 50.0, 50.0, 10.0, 4.0, 0.0, 0.0], [float("nan")] * 5 + [0.0] * 3], dtype=torch.float64)
    fit = sb.batch.pose_fit(m)
    assert abs(fit.theta[0].item() - np.pi / 4) < 1e-15 and fit.omega[0].item() == 0.2
    assert abs(fit.rms[0].item() - np.sqrt((100.0 - 2.0 * np.sqrt(1250.0)) / 4.0)) < 1e-12
    assert all(bool(torch.isnan(x[1])) for x in fit)
    exact = sb.batch.pose_fit(torch.tensor([3.0, 4.0, 5.0, 5.0, 0.0, 2.0, 0.0, 0.0], dtype=torch.float64))
    assert exact.rms.item() == 0.0 and exact.omega.item() == 0.0


# ---------------------------------------------------------------- by hand: small integers, everything exact
SQUARE = np.array([[2.0, 1.0], [6.0, 1.0], [6.0, 5.0], [2.0, 5.0], [4.0, 3.0]], "f4")   # centroid (4, 3), I0 = 4 * 8 = 32


def one_group(sb, now, ref, cap=(8, 8), vel=None):
    """pose_ref's row 0 and moments of a scene whose particles are `now` [n, 2] (velocities `vel`), all in group 0, against `ref`."""
    buf = pc.scene_of(sb, now, vel, cap)
    full = np.full((cap[0], 2), np.nan, "f4")
    full[:len(ref)] = ref
    rows, moms, rank = pr.pose_ref(buf, np.zeros(cap[0], np.int32), 2, full)
    assert rank[:len(now)].tolist() == [0] * len(now) and b32(rows[1]).tolist() == b32(pr.empty_row()).tolist()
    assert b64(moms[1]).tolist() == b64(pr.empty_moments()).tolist()
    return rows[0], moms[0]


def test_identity_translation_quarter_turn_and_a_single_particle(sb):
    row, m = one_group(sb, SQUARE, SQUARE)
    assert row[:4].tolist() == [5, 0, 5, 0] and row[4:10].tolist() == [4, 3, 4, 3, 0, 0]
    assert b64(m[1]) == 0 and b64(m[0]) == b64(m[2]) == b64(m[3]) == b64(np.float64(32.0))            # b == +0.0; a, I, I0 the same bits
    assert m[5] == 5 and row[10:17].tolist() == [32, 0, 32, 32, 0, 0, 1] and not row[17:].any() and b32(row[11]) == 0
    row, m = one_group(sb, SQUARE + np.array([100.0, -3.0], "f4"), SQUARE)                                 # pure translation: the same
    assert b64(m[1]) == 0 and b64(m[0]) == b64(m[2]) == b64(m[3]) == b64(np.float64(32.0)) and row[4:8].tolist() == [104, 0, 4, 3]
    turned = np.stack([-(SQUARE[:, 1] - 3.0) + 10.0, (SQUARE[:, 0] - 4.0) + 20.0], axis=1).astype("f4")   # a quarter turn about the centroid, shifted
    spin = np.stack([-(turned[:, 1] - 20.0), turned[:, 0] - 10.0], axis=1).astype("f4") * 2.0 + np.array([7.0, -1.0], "f4")   # omega = 2, plus a drift
    row, m = one_group(sb, turned, SQUARE, vel=spin)
    assert m[0] == 0 and b64(m[1]) == b64(m[2]) == b64(m[3]) == b64(np.float64(32.0))                      # a == 0, b == I == I0
    assert m[4] == 64 and row[14] == 64 and row[15] == 2 and row[8:10].tolist() == [7, -1] and row[16] == 1
    row, m = one_group(sb, SQUARE[:1], SQUARE[:1])
    assert m[2] == 0 and m[5] == 1 and np.isnan(row[15]) and np.isnan(row[16]) and row[12] == 0 and b32(row[15]) == 0x7FC00000
    # unmatched members are counted, not summed; none matched: NaN
    ref = SQUARE.copy()
    ref[4] = np.nan
    row, m = one_group(sb, SQUARE, ref)
    assert row[:4].tolist() == [5, 0, 4, 1] and m[5] == 4 and m[0] == m[2] == 32
    row, m = one_group(sb, SQUARE, np.full((5, 2), np.inf, "f4"))
    assert row[:4].tolist() == [5, 0, 0, 5] and np.isnan(row[4:17]).all() and not row[17:].any()
    assert b64(m).tolist() == b64(pr.empty_moments()).tolist() and b32(row[4:17]).tolist() == [0x7FC00000] * 13


# ---------------------------------------------------------------- the kernel's route against the dense trees
@pytest.mark.parametrize("W", [8, 128, 1024])
def test_the_sparse_route_gives_the_bits_of_the_masked_trees(sb, W):
    rng = np.random.default_rng(100 + W)
    maxP = W if W != 128 else 65      # (a capacity that is no power of two: leaves 65 .. 127 are never members)
    i = np.arange(maxP)
    groupings = {"random few": rng.integers(0, 3, maxP), "random many": rng.integers(0, maxP, maxP), "interleaved": i % 2,
                 "out of range": np.where(rng.random(maxP) < 0.3, rng.choice([-1, maxP, qr.INT32_MIN], maxP), rng.integers(0, 4, maxP))}
    if W == 1024:
        groupings = {k: groupings[k] for k in ("random few", "random many")}   # (the replay is quadratic)
    differs = 0
    for name, labels in groupings.items():
        # magnitudes spread over 2^40: nearly every addition rounds, so another order gives other bits
        rec = (rng.standard_normal((maxP, 6)) * (2.0 ** 40) ** rng.random((maxP, 6))).astype("f4")
        ref = (rng.standard_normal((maxP, 2)) * (2.0 ** 40) ** rng.random((maxP, 2))).astype("f4")
        ref[rng.random(maxP) < 0.1] = np.nan
        rec[rng.random(maxP) < 0.05, 2] = np.inf
        buf = pc.scene_of(sb, rec[:, :2], rec[:, 2:4], (maxP, 8))
        buf.particles[:maxP, 2] = rec[:, 2]
        labels = labels.astype(np.int32)
        rows, moms, rank = pr.pose_ref(buf, labels, maxP, ref)
        grp, ok = qr.groups_of(buf, labels), pr.matched_of(buf, ref)
        member = (grp >= 0) & ok
        leaves = np.zeros((pr.NSUM, maxP))
        leaves[:, member] = pr.leaves_of(buf.particles[member], ref[member])
        sums = [qr.replay_route(grp, member, leaves[c], W) for c in range(pr.NSUM)]
        assert 0 < member.sum() and (W == 8 or member.sum() < (grp >= 0).sum()), name   # (some are unmatched: NaN reference, inf velocity)
        for g in sorted(sums[0]):
            k = int(rank[np.nonzero(grp == g)[0][0]])
            n = int((member & (grp == g)).sum())
            row, mom = pr.empty_row(), pr.empty_moments()
            with np.errstate(all="ignore"):
                pr.fill(row, mom, [s[g] for s in sums], n)
            assert b32(row[4:17]).tolist() == b32(rows[k, 4:17]).tolist() and b64(mom).tolist() == b64(moms[k]).tolist(), (W, name, g)
            serial = np.float64(0.0)
            for x in leaves[pr.D][member & (grp == g)]:
                serial = serial + x
            differs += serial != sums[pr.D][g]
        assert set(int(x) for x in rows[:, 1] if x >= 0) >= set(sums[0]), name
    assert W == 8 or differs > 0   # and the order does matter: a sum in index order differs somewhere


# ---------------------------------------------------------------- the body summary's means
def test_centroid_and_mean_velocity_are_the_body_summarys_words(sb):
    for case in qc.graph_cases(sb)[1:]:
        maxP = case["cap"][0]
        labels = qr.body_labels_of(case["bufs"], maxP)
        refs = [pr.reference_of(b) for b in case["bufs"]]
        rows, moms, rank = pr.pose_of(case["bufs"], labels, maxP, refs)
        brows, brank = qr.body_summary_of(case["bufs"], labels, maxP)
        assert np.array_equal(rank, brank) and np.array_equal(rows[:, :, 1], brows[:, :, 2]) and np.array_equal(rows[:, :, 0], brows[:, :, 0])
        live = rows[:, :, 1] >= 0
        assert live.sum() == sum(case["groups"]) and (rows[live][:, 3] == 0).all()
        assert b32(rows[live][:, [4, 5, 8, 9]]).tolist() == b32(brows[live][:, 6:10]).tolist()
        # the reference is the scene itself: b == +0.0, a == I == I0 by bits
        assert (b64(moms[live][:, 1]) == 0).all() and (b64(moms[live][:, 0]) == b64(moms[live][:, 2])).all()
        assert (b64(moms[live][:, 2]) == b64(moms[live][:, 3])).all() and (moms[live][:, 2] > 0).all()


# ---------------------------------------------------------------- the header on the host, under sanitizers
def _records(sb):
    rng = np.random.default_rng(5)
    blob, want = [], []
    rec = (rng.standard_normal((300, 6)) * (2.0 ** 40) ** rng.random((300, 6))).astype("f4")
    rec[:20] = rng.integers(-8, 9, (20, 6)).astype("f4")
    rec[20] = 0.0
    rec[21] = -0.0
    leaves = pr.leaves_of(rec[:, [0, 1, 2, 3]], rec[:, 4:6])
    for k in range(len(rec)):
        blob.append(np.array([1] + [int(x) for x in b32(rec[k, [0, 1, 2, 3, 4, 5]])], "<u8").tobytes())
        want.append("l " + " ".join("%016x" % int(x) for x in b64(leaves[:, k])))
    for n in (1, 2, 3, 7, 64, 1024):
        for scale in (1.0, 2.0 ** 20):
            for _ in range(20):
                m = (rng.standard_normal((n, 6)) * scale ** rng.random((n, 6))).astype("f4")
                if _ % 5 == 0:
                    m[:, 4:6] = m[:, 0:2]                      # the reference is the shape: I == I0
                if _ % 5 == 1:
                    m[:, 0:2] = m[0, 0:2]                      # all in one point: I == 0
                S = pr.leaves_of(m[:, :4], m[:, 4:6]).sum(axis=1) + 0.0
                row, mom = pr.empty_row(), pr.empty_moments()
                with np.errstate(all="ignore"):
                    pr.fill(row, mom, S, n)
                blob.append(np.array([2], "<u8").tobytes() + S.astype("<f8").tobytes() + np.array([n], "<f8").tobytes())
                want.append("f " + " ".join("%08x" % int(x) for x in b32(row[4:17])) + " " + " ".join("%016x" % int(x) for x in b64(mom)))
    blob.append(np.array([3], "<u8").tobytes())
    want.append("u " + " ".join("%08x" % int(x) for x in b32(pr.empty_row()[4:])) + " " + " ".join("%016x" % int(x) for x in b64(pr.empty_moments())))
    return b"".join(blob), want


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_header_equals_the_restatement_under_sanitizers(sb, tmp_path, san):
    target = os.path.join("hostcheck_build", "batch_pose_check_" + san)
    p = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    blob, want = _records(sb)
    path = str(tmp_path / "records.bin")
    with open(path, "wb") as f:
        f.write(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(CSRC, target), path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want) > 500
    bad = [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]          # exact: both sides are this CPU's
    assert not bad, bad[:5]


# ---------------------------------------------------------------- the geometric property, on the restatement
def test_the_turned_lattice_gives_its_angle_within_the_bounds(sb):
    g = pc.turned_lattice(sb)
    rows, moms, rank = pr.pose_ref(g["buf"], np.zeros(g["cap"][0], np.int32), 1, g["ref"])
    assert rows[0, :4].tolist() == [64, 0, 64, 0] and 12.9 < g["r_rms"] < 13.1 and g["delta"] < 5.4e-6
    theta = np.arctan2(np.float64(rows[0, 11]), np.float64(rows[0, 10]))
    assert abs(theta - pc.THETA) <= g["theta_bound"] < 1.1e-6, (theta, g["theta_bound"])
    a, b, i, i0, lc, n = moms[0, :6]
    rms = np.sqrt(max(i + i0 - 2.0 * np.sqrt(a * a + b * b), 0.0) / n)
    assert rms <= pc.RMS_BOUND, rms
    assert abs(rows[0, 16] - 1.0) < 1e-5 and rows[0, 15] == 0


# ---------------------------------------------------------------- the programs of the GPU tests, on the oracle
@pytest.fixture(scope="module")
def expected(sb, oracle):
    return {c["name"]: (c, qc.expected(oracle, c)[0]) for c in pc.stepped_cases(sb)}


def test_the_recorded_figures(sb, expected):
    case, exp = expected["default scene at 120 / 300"]
    now, labels, pending = exp[0]
    rows, moms, rank = pr.pose_of(now, labels, 8, [pr.reference_of(b) for b in case["bufs"]])
    brows, brank = qr.body_summary_of(now, labels, 8, pending)
    assert rows[0, :, 0].tolist() == [40, 36, 25, 4, 4, 4, 4, 1] and (rows[0, :, 3] == 0).all() and np.array_equal(rank, brank)
    assert b32(rows[0][:, [4, 5, 8, 9]]).tolist() == b32(brows[0][:, 6:10]).tolist()
    assert np.isnan(rows[0, 7, 15]) and np.isnan(rows[0, 7, 16]) and moms[0, 7, 2] == 0          # a body of one particle
    assert np.isfinite(rows[0, :7]).all() and (np.abs(rows[0, :7, 16] - 1.0) < 0.2).all()       # two frames in: nearly rigid still
    case, exp = expected["yield / break / delete"]
    for k in case["compare_after"]:
        now, labels, pending = exp[k]
        rows, moms, rank = pr.pose_of(now, labels, 4, [pr.reference_of(b) for b in case["bufs"]])
        assert rows[:, 0, 0].tolist() == [144, 139, 120, 101, 84, 144] and (rows[:, :, 3] == 0).all()
        assert (moms[:, 0, 0] > 0).all() and (np.abs(np.arctan2(moms[:, 0, 1], moms[:, 0, 0])) < 0.5).all()
    case, exp = expected["force saturation"]
    k = case["compare_after"][0]
    now, labels, pending = exp[k]
    refs = [pr.reference_of(b) for b in case["bufs"]]
    N = qc.nonfinite_labels(len(now))
    rows, moms, rank = pr.pose_of(now, N["one group"], 2, refs)
    bad = rows[pc.NONFINITE_SCENE]
    assert bad[0, :4].tolist() == [6, 0, 4, 2] and np.isfinite(bad[0]).all() and bad[1, 1] == -1
    rows, moms, rank = pr.pose_of(now, N["non-finite apart"], 2, refs)
    bad = rows[pc.NONFINITE_SCENE]
    assert bad[:, :4].tolist() == [[4, 0, 4, 0], [2, 3, 0, 2]] and np.isnan(bad[1, 4:17]).all() and np.isnan(moms[pc.NONFINITE_SCENE, 1, :5]).all()
    assert len(expected) == 3


def test_the_graphs_and_the_callers_reference(sb):
    case = qc.case_limit(sb)
    maxP = case["cap"][0]
    labels = qr.body_labels_of(case["bufs"], maxP)
    refs = pc.caller_refs(case["bufs"], maxP)
    rows, moms, rank = pr.pose_of(case["bufs"], labels, 16, refs)
    assert rows[0, 0, :4].tolist() == [1024, rows[0, 0, 1], 1024 - rows[0, 0, 3], rows[0, 0, 3]] and 50 < rows[0, 0, 3] < 200
    assert (rows[1, :, 0] == 64).all() and (np.diff(rows[1, :, 1]) > 0).all() and rows[1, :, 3].sum() > 0
    assert rows[2, :, 0].tolist() == [2] * 16 and set(rows[2, :, 2].tolist()) <= {0.0, 1.0, 2.0}
    assert b32(rows[5]).tolist() == b32(rows[6]).tolist() == [b32(pr.empty_row()).tolist()] * 16
    assert (rank[5:] == -1).all() and (rank[2] >= 16).sum() == 1024 - 32
