"""sb_batch_add_particles_device without a GPU: softbody.h declares it and the library exports it, batch.py binds it, the row struct
is 32 bytes and the SB_BATCH_SPAWN_* constants agree between the header and Python, the argument checks come before any device
call; tests/batch_add_particles_ref.py on every case of tests/batch_add_particles_cases.py: every row code, the three cases of the
blocked rule, room, the smallest free index with an out-of-order mapping, the reset rule; the edited buffers load into the oracle
and do what the case says; csrc/sb_batch_spawn_math.h (built on the host, under sanitizers) agrees with the restatement."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import batch_add_particles_cases as cases
import batch_add_particles_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbody-webgpu_amd", "csrc")
ERR_INVALID = 1
SYMBOL = "sb_batch_add_particles_device"
E, I, B, FULL = ref.EMPTY, ref.INVALID, ref.BLOCKED, ref.FULL


def test_header_declares_and_library_exports(sb):
    assert SYMBOL in sb.engine.declared_symbols()
    L = sb.engine.load_library()
    assert hasattr(L, SYMBOL) and L.sb_abi_version() == 1
    bl = sb.batch.load_library()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert bl.sb_batch_add_particles_device.argtypes == [vp, u32, vp, u32, vp, vp] and bl.sb_batch_add_particles_device.restype is ctypes.c_int
    assert callable(sb.BatchEngine.add_particles) and callable(sb.batch.new_particle_rows) and callable(sb.batch.body_beam_rows)


def test_struct_and_constants(sb):
    src = open(sb.engine.HEADER_PATH).read()
    assert "#define SB_ABI_VERSION 1\n" in src
    m = re.search(r"typedef struct sb_batch_new_particle \{(.*?)\} sb_batch_new_particle;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int32_t|uint32_t|float)\s+([^;]+);", body):
        fields += [(ctype, n.strip()) for n in names.split(",")]
    assert fields == [("int32_t", "tag")] + [("float", n) for n in ("x", "y", "vx", "vy", "ax", "ay")] + [("uint32_t", "reserved")]
    b = sb.batch
    assert 4 * len(fields) == 32 == 4 * b.SPAWN_ROW_WORDS == 4 * ref.ROW_WORDS
    got = dict(re.findall(r"#define SB_BATCH_SPAWN_(\w+)\s+\(?(-?\d+)u?\)?", src))
    assert {k: int(v) for k, v in got.items()} == {
        "DRY_RUN": b.SPAWN_DRY_RUN, "SKIP_TOUCHING": b.SPAWN_SKIP_TOUCHING, "EMPTY": b.SPAWN_EMPTY, "INVALID": b.SPAWN_INVALID,
        "BLOCKED": b.SPAWN_BLOCKED, "FULL": b.SPAWN_FULL, "COUNT_WORDS": len(b.SPAWN_COUNT_FIELDS)}
    assert (b.SPAWN_DRY_RUN, b.SPAWN_SKIP_TOUCHING) == (1, 2) == (ref.DRY_RUN, ref.SKIP_TOUCHING)
    assert (b.SPAWN_EMPTY, b.SPAWN_INVALID, b.SPAWN_BLOCKED, b.SPAWN_FULL) == (-1, -2, -3, -4) == (E, I, B, FULL)
    assert b.SPAWN_COUNT_FIELDS == ("added", "invalid", "blocked", "full") == sb.SPAWN_COUNT_FIELDS and sb.SPAWN_BLOCKED == -3
    for needle in ("add_particles_kernel_vgprs", "add_particles_kernel_scratch_bytes"):
        assert needle in src, needle


def test_null_handle_is_refused_without_a_device(sb):
    """every INVALID case of the header on a NULL handle: nothing may touch a device on the way"""
    L = sb.batch.load_library()
    p = ctypes.c_void_p(4096)
    for flags, rows, k, result, counts in ((0, p, 1, None, None), (4, p, 1, None, None), (0, p, 65, None, None), (0, None, 1, None, None),
                                           (0, ctypes.c_void_p(4097), 1, None, None), (0, p, 1, ctypes.c_void_p(4098), None),
                                           (0, p, 1, None, ctypes.c_void_p(4099)), (0, None, 0, None, None)):
        assert L.sb_batch_add_particles_device(None, flags, rows, k, result, counts) == ERR_INVALID


# ---------------------------------------------------------------- the restatement on the cases

def oracle_run(oracle, buf, frames=2, mode=1):
    r = oracle.OracleEngine(1000.0, 10.0, 64, buf.layout, mode, threads=2)
    r.write_buffers(buf)
    for _ in range(frames):
        r.frame()
    out = r.load_buffers(buf.copy())
    assert np.isfinite(out.particles[buf.mapping[:buf.particle_count].astype(np.int64)]).all()
    return out


def test_default_case(sb, oracle):
    """each scene adds three particles; inside two frames the first bounces off the left wall and the second is pushed by the body"""
    case = cases.default_case(sb)
    exp = cases.expected(case)
    assert len({r.tobytes() for r in case["rows"]}) == len(exp), "every scene its own rows"
    for i, (edited, res, counts) in enumerate(exp):
        assert res[:3].tolist() == [119, 120, 121] and res[3] == (E if i % 4 == 0 else I) and counts == [3, int(i % 4 != 0), 0, 0]
        assert edited.particle_count == 122 and edited.mapping[119:122].tolist() == [119, 120, 121]
        assert edited.particles[119:122].tobytes() == case["rows"][i][:3, 1:7].tobytes()
        on, off = oracle_run(oracle, edited, mode=1), oracle_run(oracle, edited, mode=0)
        assert on.particles[119, 2] > 0.0 and off.particles[119, 2] > 0.0, "the wall turned the first particle round"
        assert on.particles[120].tobytes() != off.particles[120].tobytes(), "contacts act on the second"
        assert on.particles[1].tobytes() != off.particles[1].tobytes(), "and on the particle it fell on"


def test_codes_case_and_the_blocked_rule(sb):
    case = cases.codes_case(sb)
    buf, rows = case["bufs"][0], case["rows"][0]
    pos = rows[:, 1:3].copy().view("f4")
    # the coordinates give exactly 2r, and one ulp less, in the contact test's own arithmetic
    with np.errstate(all="ignore"):
        d0 = np.sqrt(np.float32((buf.particles[1, 0] - pos[0, 0]) ** 2 + (buf.particles[1, 1] - pos[0, 1]) ** 2), dtype="f4")
        d1 = np.sqrt(np.float32((buf.particles[3, 0] - pos[1, 0]) ** 2 + (buf.particles[3, 1] - pos[1, 1]) ** 2), dtype="f4")
    assert d0 == np.float32(20.0) and d1 < np.float32(20.0) and cases.step_ulps(float(pos[1, 0]), 1) == 265.0 == float(buf.particles[3, 0]) + 20.0
    assert not ref.touch(pos[0], buf.particles[1], 10.0) and ref.touch(pos[1], buf.particles[3], 10.0) and ref.touch(pos[2], buf.particles[1], 10.0)
    (edited, res, counts), = cases.expected(case)
    assert res.tolist() == [119, B, B, I, I, I, I, E, 120, B, B, B, 121, 122, 123] and counts == [5, 4, 5, 0]
    # the three cases of the rule: an existing particle (1, 2, 11), an earlier clean row (9; 10 by a row that was itself blocked by a
    # row), an earlier row that is E and therefore does not block (12 touches 11 alone)
    assert ref.touch(pos[9], pos[8], 10.0) and ref.touch(pos[10], pos[9], 10.0) and not ref.touch(pos[10], pos[8], 10.0)
    assert ref.touch(pos[12], pos[11], 10.0) and not any(ref.touch(pos[12], pos[i], 10.0) for i in (0, 1, 2, 8, 9, 10))
    here = buf.particles[:119, :2]
    assert not any(ref.touch(pos[j], q, 10.0) for j in (0, 8, 9, 10, 12) for q in here)
    assert edited.particles[120].view("u4").tolist() == rows[8, 1:7].view(np.uint32).tolist(), "non-finite velocity taken verbatim"
    (_, res, counts), = cases.expected(case, flags=0)
    assert res.tolist() == [119, 120, 121, I, I, I, I, E, 122, 123, 124, 125, 126, 127, FULL] and counts == [9, 4, 0, 1]
    (same, res2, counts2), = cases.expected(case, flags=ref.DRY_RUN)
    assert same is buf and res2.tolist() == res.tolist() and counts2 == counts


def test_room_and_sparse_cases(sb, oracle):
    exp = cases.expected(cases.room_case(sb))
    assert exp[0][1].tolist() == [16, 17, 18, FULL, E, FULL] and exp[0][2] == [3, 0, 0, 2] and exp[0][0].particle_count == 19
    assert exp[1][1].tolist() == [FULL] * 4 + [E, FULL] and exp[1][2] == [0, 0, 0, 5]
    assert exp[2][0] is None and exp[2][1].tolist() == [I] * 4 + [E, I] and exp[2][2] == [0, 5, 0, 0]
    oracle_run(oracle, exp[0][0])
    case = cases.sparse_case(sb)
    buf = case["bufs"][0]
    (edited, res, counts), = cases.expected(case)
    used = set(((5 * np.arange(16) + 2) % 32).tolist())
    assert res.tolist() == [d for d in range(32) if d not in used][:3] == [1, 4, 6] and counts == [3, 0, 0, 0]
    assert buf.particle_count == 16 and 16 not in res.tolist() and ref.held(buf)[17]
    assert edited.mapping[16:19].tolist() == [1, 4, 6] and edited.mapping[:16].tolist() == buf.mapping[:16].tolist()
    oracle_run(oracle, edited)


def test_reset_rule(sb):
    """spawn, reset, spawn on the triple: the reset gives the indices back and the same spawn takes them again"""
    case = cases.sparse_case(sb)
    buf = case["bufs"][0]
    edited, res, _ = ref.add_ref(buf, case["rows"][0])
    back, held = ref.reset_ref(edited, buf, 16)
    assert back.particle_count == 16 and not held[[1, 4, 6]].any() and held.sum() == 16
    assert back.mapping[16:19].tolist() == [1, 4, 6], "the stale entries of the constant mapping stay"
    assert back.particles.tobytes() == buf.particles.tobytes() and back.beams.tobytes() == buf.beams.tobytes()
    again, res2, _ = ref.add_ref(back, case["rows"][0])
    assert res2.tolist() == res.tolist() and again.particles.tobytes() == edited.particles.tobytes() and again.mapping.tobytes() == edited.mapping.tobytes()
    # a checkpoint in between keeps them: the triple's p0 is then the new count
    kept, held = ref.reset_ref(edited, edited, 19)
    assert kept.particle_count == 19 and held[[1, 4, 6]].all()


def test_width_cases(sb, oracle):
    """what each case of the width file is named for, on the restatement alone"""
    case = cases.sixty_four_case(sb)
    exp = cases.expected(case)
    free = sorted(list(range(972, 1024)) + list(range(0, 64, 2))[:12])
    assert exp[0][1].tolist() == free and exp[0][2] == [64, 0, 0, 0] and exp[0][0].particle_count == 1024
    assert sum(d >= 992 for d in free) == 32, "the last bitmap word is all free"
    assert exp[1][2] == [24, 0, 0, 40] and exp[1][1][24:].tolist() == [FULL] * 40 and exp[1][0].particle_count == 1024
    case = cases.threshold_case(sb)
    (edited, res, counts), = cases.expected(case)
    assert case["bufs"][0].particle_count == 250 < 256 <= edited.particle_count == 260 and counts == [10, 0, 0, 0]
    for cap in cases.ODD_CAPS:
        case = cases.odd_case(sb, cap)
        exp = cases.expected(case)
        assert exp[0][2] == exp[2][2] == [0, 0, 0, 0] and exp[1][2] == [cap[0] - 25, 0, 0, 2]
        assert exp[1][1][-3] == max(d for d in range(cap[0]) if not ref.held(case["bufs"][1])[d]) and exp[1][0].particle_count == cap[0]
        oracle_run(oracle, exp[1][0], frames=1)
    case = cases.halves_case(sb)
    (edited, res, counts), = cases.expected(case)
    assert res.tolist() == list(range(16, 48)) + [B] * 32 and counts == [32, 0, 32, 0]
    pos = case["rows"][0][:, 1:3].copy().view("f4")
    for j in range(32):
        assert [i for i in range(32 + j) if ref.touch(pos[32 + j], pos[i], 10.0)] == [j]


# ---------------------------------------------------------------- the row verdict and the contact test: header == restatement

@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_header_equals_the_restatement_under_sanitizers(sb, tmp_path, san):
    """csrc/sb_batch_spawn_math.h on the host (tests/batch_spawn_check.cpp, `make hostcheck`) == batch_add_particles_ref.row_verdict
    and .touch: the rows of the codes case as one group (with its blocked column), then random rows with special coordinates, at
    distances round 2r to the ulp, and with radii whose threshold is no ordinary number"""
    exe = os.path.join(CSRC, "hostcheck_build", "batch_spawn_check_" + san)
    p = subprocess.run(["make", "-C", CSRC, os.path.join("hostcheck_build", "batch_spawn_check_" + san)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    rng = np.random.default_rng(12)
    case = cases.codes_case(sb)
    buf, rows = case["bufs"][0], case["rows"][0]
    here = buf.particles[:119, :2]
    recs = []
    for row in rows:       # the group: `other` is a particle the row touches where there is one (E), else particle 0
        pos = row[1:3].copy().view("f4")
        hit = [q for q in here if ref.row_verdict(row, True) == 0 and ref.touch(pos, q, 10.0)]
        recs.append((row, 1, 10.0, hit[0] if hit else here[0]))
    group = len(recs)
    special = np.asarray([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, 3.4028235e38, -1.0, 1.0e20], "f4")
    for _ in range(4000):
        row = np.zeros(8, np.int32)
        row[0] = rng.integers(-2, 6)
        xy = (rng.normal(size=2) * 300).astype("f4")
        if rng.random() < 0.3:
            xy[rng.integers(2)] = special[rng.integers(len(special))]
        row[1:3] = xy.view(np.int32)
        row[7] = int(rng.random() < 0.1)
        radius = np.float32([10.0, 10.0, 10.0, 0.3, 1e-30, 1e30, np.nan, 0.0][rng.integers(8)])
        u = rng.random()
        if u < 0.4:       # round 2r, to the ulp
            t = rng.uniform(0, 2 * np.pi)
            other = (xy + np.float32(2 * radius) * np.asarray([np.cos(t), np.sin(t)], "f4")).astype("f4")
            other[0] = cases.step_ulps(abs(float(other[0])) or 1.0, int(rng.integers(-3, 4))) * (1 if other[0] >= 0 else -1) if np.isfinite(other[0]) else other[0]
        elif u < 0.5:
            other = xy.copy()
        else:
            other = (rng.normal(size=2) * 300).astype("f4")
        recs.append((row, int(rng.random() < 0.9), radius, other))
    words = np.zeros((len(recs), 12), "<u4")
    want = []
    for i, (row, loaded, radius, other) in enumerate(recs):
        words[i, :8] = np.asarray(row, np.int32).view(np.uint32)
        words[i, 8] = loaded
        words[i, 9] = np.float32(radius).view(np.uint32)
        words[i, 10:12] = np.asarray(other, "f4").view(np.uint32)
        want.append("%d %d" % (ref.row_verdict(row, bool(loaded)), int(ref.touch(np.asarray(row[1:3], np.int32).view("f4"), other, radius))))
    (_, res, _), = cases.expected(case)
    want.append(" ".join(str(int(c == B)) for c in res))
    path = str(tmp_path / "records.bin")
    words.tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, path, str(group)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, [(i, got[i], want[i]) for i in bad[:5]]
    codes = [int(w.split()[0]) for w in want[:-1]]
    touches = [int(w.split()[1]) for w in want[:-1]]
    assert min(codes.count(c) for c in (0, E, I)) > 100 and min(touches.count(t) for t in (0, 1)) > 300


# ---------------------------------------------------------------- the row packers (torch ops; here on CPU tensors)

def test_new_particle_rows_and_body_beam_rows(sb):
    import torch
    import batch_add_beams_ref as beam_ref
    pos = torch.tensor([[[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], [[7.0, 8.0], [9.0, 10.0], [11.0, 12.0]]])
    vel, acc = torch.tensor([0.5, -0.5]), torch.tensor([[[0.0, 1.0]], [[2.0, float("nan")]]])       # broadcast over [N, k] and over k
    valid = torch.tensor([True, False, True])                                                        # broadcast over N
    rows = sb.batch.new_particle_rows(pos, vel, acc, valid).numpy()
    want = np.stack([ref.pack([(0 if valid[j] else -1, *pos[i, j].tolist(), 0.5, -0.5, *acc[i, 0].tolist()) for j in range(3)]) for i in range(2)])
    assert rows.dtype == np.int32 and rows.tobytes() == want.tobytes()
    assert sb.batch.new_particle_rows(pos).numpy().tobytes() == np.stack(
        [ref.pack([(0, *pos[i, j].tolist()) for j in range(3)]) for i in range(2)]).tobytes()
    with pytest.raises(ValueError):
        sb.batch.new_particle_rows(pos.double())
    result = torch.tensor([[20, 21, 22], [5, ref.FULL, 7]], dtype=torch.int32)
    edges = [(0, 1), (1, 2), (2, 0)]
    mat = (1.0, 50.0, 1.0, 2.5)
    got = sb.batch.body_beam_rows(result, edges, 30.0, *mat).numpy()
    want = np.stack([beam_ref.pack([(20, 21, 30.0) + mat, (21, 22, 30.0) + mat, (22, 20, 30.0) + mat]),
                     beam_ref.pack([(-1, -1, 30.0) + mat, (-1, -1, 30.0) + mat, (7, 5, 30.0) + mat])])
    assert got.tobytes() == want.tobytes()
    assert sb.batch.body_beam_rows(result, torch.tensor(edges), 30.0, *mat).numpy().tobytes() == want.tobytes()
    for bad in ([(0, 3)], [(-1, 0)], [(0, 1, 2)]):
        with pytest.raises(ValueError):
            sb.batch.body_beam_rows(result, bad, 30.0, *mat)
