"""sb_cut_device / sb_cut / sb_batch_cut_device without a GPU: softbody.h declares them, engine.py and batch.py bind them with
prototypes, the SB_CUT_* constants agree between the header and Python, the argument checks that come before any device call; the
predicate: tests/cut_ref.py (numpy float32) against the exact geometry in fractions and against the case table, csrc/sb_cut_math.h
(built on the host, under sanitizers) against cut_ref; and every scene case of the GPU tests hits something and misses something."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cut_cases
import cut_ref

SYMBOLS = ["sb_cut_device", "sb_cut", "sb_batch_cut_device"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbody-webgpu_amd", "csrc")
ERR_INVALID = 1


def test_header_declares_the_calls(sb):
    names = sb.engine.declared_symbols()
    for s in SYMBOLS:
        assert s in names, s
    L = sb.engine.load_library()
    for s in SYMBOLS:
        assert hasattr(L, s), s


def test_constants_agree(sb):
    src = open(sb.engine.HEADER_PATH).read()
    got = {n: int(v) for n, v in re.findall(r"#define SB_CUT_(\w+)\s+(\d+)u", src)}
    e = sb.engine
    assert got == {"NONE": e.CUT_NONE, "SEGMENT": e.CUT_SEGMENT, "DISC": e.CUT_DISC, "MAX_SHAPES": e.CUT_MAX_SHAPES,
                   "COUNT_WORDS": len(e.CUT_COUNT_FIELDS), "DRY_RUN": e.CUT_DRY_RUN}
    assert (e.CUT_NONE, e.CUT_SEGMENT, e.CUT_DISC, e.CUT_MAX_SHAPES, e.CUT_DRY_RUN) == (0, 1, 2, 64, 1)
    assert e.CUT_COUNT_FIELDS == ("tested", "hit", "flagged", "already_flagged")
    assert (cut_ref.NONE, cut_ref.SEGMENT, cut_ref.DISC) == (e.CUT_NONE, e.CUT_SEGMENT, e.CUT_DISC)
    assert (sb.CUT_NONE, sb.CUT_SEGMENT, sb.CUT_DISC, sb.CUT_COUNT_FIELDS) == (0, 1, 2, e.CUT_COUNT_FIELDS) and sb.cut_shapes is e.cut_shapes
    assert ctypes.sizeof(e.SbCutOptions) == 32
    m = re.search(r"typedef struct sb_cut_options \{(.*?)\} sb_cut_options;", src, re.S)
    assert re.findall(r"uint32_t (\w+)", m.group(1)) == ["struct_size", "flags", "reserved"]
    assert "#define SB_ABI_VERSION 1\n" in src and ctypes.sizeof(e.SbOptions) == 64


def test_bindings(sb):
    L = sb.engine.load_library()
    sb.batch.load_library()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    opts = ctypes.POINTER(sb.engine.SbCutOptions)
    assert L.sb_cut_device.argtypes == [vp, opts, vp, u32, vp, vp] and L.sb_cut.argtypes == [vp, opts, vp, u32, vp, vp]
    assert L.sb_batch_cut_device.argtypes == [vp, u32, vp, u32, vp, vp]
    for s in SYMBOLS:
        assert getattr(L, s).restype is ctypes.c_int
    assert callable(sb.Engine.cut) and callable(sb.BatchEngine.cut)


def test_null_handles_are_refused_without_a_device(sb):
    """every INVALID case of the header on a NULL handle: nothing may touch a device on the way"""
    L = sb.engine.load_library()
    sb.batch.load_library()
    p = ctypes.c_void_p(4096)
    o = sb.engine.SbCutOptions()
    for size, flags, reserved in ((31, 0, 0), (32, 2, 0), (32, 0, 1), (0, 0, 0), (32, 1, 0)):
        o.struct_size, o.flags, o.reserved[0] = size, flags, reserved
        for call in (L.sb_cut_device, L.sb_cut):
            for shapes, n, counts in ((p, 1, None), (p, 65, None), (None, 1, None), (ctypes.c_void_p(4098), 1, None), (p, 1, ctypes.c_void_p(4100))):
                assert call(None, ctypes.byref(o), shapes, n, None, counts) == ERR_INVALID
    for flags, shapes, k, counts in ((0, p, 1, None), (2, p, 1, None), (0, p, 65, None), (0, None, 1, None), (0, ctypes.c_void_p(4097), 1, None),
                                     (0, p, 1, ctypes.c_void_p(4098))):
        assert L.sb_batch_cut_device(None, flags, shapes, k, None, counts) == ERR_INVALID


def test_shape_packing(sb):
    e = sb.engine
    rows = e.cut_shapes(segments=[(0, 1, 2, 3)], discs=[(4, 5, 6)])
    assert rows.dtype == np.uint32 and rows.shape == (2, 8)
    assert rows.tobytes() == cut_ref.pack([(1, 0, 1, 2, 3), (2, 4, 5, 6, 0)]).tobytes()
    assert e.host_shapes([(1, 0, 1, 2, 3), (2, 4, 5, 6, 0)]).tobytes() == rows.tobytes()
    assert e.host_shapes(rows).tobytes() == rows.tobytes() and e.host_shapes(rows.view(np.int32)).tobytes() == rows.tobytes()
    assert e.host_shapes(np.asarray([(1, 0, 1, 2, 3, 0, 0, 0)], dtype=np.float32)).tobytes() == rows[:1].tobytes()
    assert e.host_shapes([]).shape == (0, 8) and e.cut_shapes().shape == (0, 8)
    for bad in ([(3, 0, 0, 1, 1)], [(1, 0, 0, 1)], [(0.5, 0, 0, 1, 1)]):
        with pytest.raises(ValueError):
            e.host_shapes(bad)


# ---------------------------------------------------------------- the predicate

def one(shape, A, B):
    return bool(cut_ref.hits(cut_ref.pack([shape]), [A], [B])[0])


@pytest.mark.parametrize("case", cut_cases.TABLE, ids=[c[0] for c in cut_cases.TABLE])
def test_case_table(case):
    name, shape, A, B, expected = case
    got = one(shape, A, B)
    if expected is not None:
        assert got == expected, name
    if shape[0] == cut_ref.SEGMENT:   # which end is which does not matter to a knife
        assert one((shape[0], shape[3], shape[4], shape[1], shape[2]), A, B) == got == one(shape, B, A), name


def test_exact_rows_agree_with_the_geometry():
    for name, shape, A, B, expected in cut_cases.TABLE[:cut_cases.EXACT]:
        if name != "disc an ulp short of tangent":   # (its radius is no small number; the fractions take it as it is all the same)
            assert all(float(v) * 2 == int(float(v) * 2) for v in shape[1:] + tuple(A) + tuple(B)), name
        assert cut_ref.exact_hit(shape, A, B) == expected == one(shape, A, B), name


def test_reference_equals_the_exact_predicate_on_halves():
    """coordinates in {-4, -3.5 .. 4}: every float32 operation of the predicate is exact, so the two must agree on every case"""
    rng = np.random.default_rng(5)
    n = 6000
    xy = rng.integers(-8, 9, size=(n, 9)).astype(np.float32) / np.float32(2.0)
    kinds = rng.integers(1, 3, size=n)
    collinear = rng.random(n) < 0.3   # the measure-zero cases, often: the knife's ends on the beam's line
    hit_count = 0
    for i in range(n):
        x0, y0, x1, y1, ax, ay, bx, by, r = (float(v) for v in xy[i])
        if kinds[i] == cut_ref.DISC:
            shape = (cut_ref.DISC, x0, y0, abs(r) / 2 if i % 7 else r, 0.0)
        else:
            if collinear[i]:
                s, t = (float(v) for v in rng.integers(-2, 4, size=2) / 2.0)
                x0, y0, x1, y1 = ax + s * (bx - ax), ay + s * (by - ay), ax + t * (bx - ax), ay + t * (by - ay)
            shape = (cut_ref.SEGMENT, x0, y0, x1, y1)
        got = one(shape, (ax, ay), (bx, by))
        assert got == cut_ref.exact_hit(shape, (ax, ay), (bx, by)), (shape, (ax, ay), (bx, by))
        hit_count += got
    assert n // 10 < hit_count < n - n // 10, hit_count


def test_any_shape_of_the_call_hits():
    shapes, A, B = cut_cases.table_arrays()
    each = np.stack([cut_ref.hits(shapes[k:k + 1], A, B) for k in range(len(shapes))])
    assert np.array_equal(cut_ref.hits(shapes, A, B), each.any(axis=0))
    assert not cut_ref.hits(shapes[:0], A, B).any()
    odd = cut_ref.pack([(3, 0, -1, 0, 1), (cut_ref.DISC, 0, 0, 10, 1)])   # an unknown kind; a disc with y1 != 0: ignored
    assert not cut_ref.hits(odd, A, B).any()


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_header_equals_the_reference_under_sanitizers(tmp_path, san):
    """csrc/sb_cut_math.h on the host (tests/cut_check.cpp, `make hostcheck`) == cut_ref on every shape of the table against every
    beam of the table, on random floats, and on shapes the device variant must ignore"""
    exe = os.path.join(CSRC, "hostcheck_build", "cut_check_" + san)
    p = subprocess.run(["make", "-C", CSRC, os.path.join("hostcheck_build", "cut_check_" + san)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    shapes, A, B = cut_cases.table_arrays()
    n = len(shapes)
    rng = np.random.default_rng(9)
    m = 4000
    rs = np.zeros((m, 8), dtype=np.uint32)
    rs[:, 0] = rng.integers(0, 4, size=m)
    rs[:, 1:5] = (rng.normal(size=(m, 4)) * 3).astype(np.float32).view(np.uint32)
    rs[::3, 4] = 0                      # (discs need y1 == 0 to count)
    rs[::5, 3] = np.abs(rs[::5, 3].view(np.float32)).view(np.uint32)
    rA, rB = (rng.normal(size=(m, 2)) * 3).astype(np.float32), (rng.normal(size=(m, 2)) * 3).astype(np.float32)
    S = np.concatenate([np.repeat(shapes, n, axis=0), rs])
    AA, BB = np.concatenate([np.tile(A, (n, 1)), rA]), np.concatenate([np.tile(B, (n, 1)), rB])
    rec = np.concatenate([S, AA.view(np.uint32), BB.view(np.uint32)], axis=1).astype("<u4")
    path = str(tmp_path / "records.bin")
    rec.tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    got = np.frombuffer(r.stdout.encode(), dtype=np.uint8) == ord("1")
    want = np.asarray([cut_ref.hits(S[i:i + 1], AA[i:i + 1], BB[i:i + 1])[0] for i in range(len(S))])
    assert len(got) == len(want) and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert 100 < want[n * n:].sum() < m - 100


# ---------------------------------------------------------------- the scene cases of the GPU tests are not vacuous

def test_every_scene_case_hits_and_misses(sb):
    for sname, make in cut_cases.SCENES.items():
        buf, _ = make(sb)
        for cname, shapes in cut_cases.scene_shapes(cut_cases.box_of(buf)).items():
            hit, counts = cut_ref.scene_ref(buf, shapes)
            assert 0 < counts[1] < counts[0] == buf.beam_count, (sname, cname, counts)
            assert hit.sum() == counts[1]


def test_every_batch_scene_case_hits_and_misses(sb):
    bufs, shapes = cut_cases.batch_scenes(sb)
    cut = 0
    for i, (buf, sh) in enumerate(zip(bufs, shapes)):
        if buf is None or not (sh[:, 0] != 0).any():
            continue
        _, counts = cut_ref.scene_ref(buf, sh)
        assert 0 < counts[1] < counts[0], (i, counts)
        cut += 1
    assert cut >= 5
