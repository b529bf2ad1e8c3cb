"""Engine.summary() (sb_summary / sb_summary_device) without a GPU: the header declares the calls, the library
exports them, engine.py binds them with prototypes and a structure of the C struct's size, bad arguments are refused before
anything touches a device, and every program of tests/test_gpu_summary.py runs on the oracle without a warning and BITES."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_summary_ref as sr  # noqa: E402
import summary_cases as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sb_summary", "sb_summary_device"]


def word(sb, name):
    return sb.engine.SUMMARY_FIELDS.index(name)


def test_header_declares_and_library_exports_the_calls(sb):
    names = sb.engine.declared_symbols()
    L = sb.engine.load_library()
    for s in SYMBOLS:
        assert s in names, s
        assert hasattr(L, s), s
    assert L.sb_abi_version() == 1   # additions only
    vp, po = ctypes.c_void_p, ctypes.POINTER(sb.engine.SbSummaryOptions)
    assert L.sb_summary_device.argtypes == [vp, po, vp, vp] and L.sb_summary.argtypes == [vp, po, vp, vp]
    assert callable(sb.Engine.summary) and callable(sb.Engine.summary_host)


def test_options_structure_and_words_are_the_c_headers(sb, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "softbody.h"\n'
                   'int main(void) { printf("%zu %zu %zu %u %u %u\\n", sizeof(sb_summary_options), offsetof(sb_summary_options, partials), '
                   'offsetof(sb_summary_options, reserved), SB_SUMMARY_WORDS, SB_BATCH_SUMMARY_WORDS, SB_SUMMARY_MAX_PARTIALS); return 0; }\n')
    exe = str(tmp_path / "size")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    size, o_partials, o_reserved, words, batch_words, cap = (int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split())
    O = sb.engine.SbSummaryOptions
    assert ctypes.sizeof(O) == size == 32
    assert (O.partials.offset, O.reserved.offset) == (o_partials, o_reserved)
    assert words == batch_words == sb.engine.SUMMARY_WORDS == len(sb.engine.SUMMARY_FIELDS) == sr.WORDS
    assert cap == 262144


def test_field_names_are_the_batchs_not_a_copy(sb):
    assert sb.engine.SUMMARY_FIELDS is sb.batch.SUMMARY_FIELDS
    assert sb.engine.SUMMARY_COUNT_FIELDS[:6] == sb.batch.SUMMARY_FIELDS[:6]


def test_null_handle_is_invalid_before_anything_touches_a_device(sb):
    L = sb.engine.load_library()
    row, counts = (ctypes.c_float * 24)(), (ctypes.c_uint64 * 8)()
    o = sb.engine.SbSummaryOptions()
    o.struct_size = ctypes.sizeof(o)
    vp = ctypes.c_void_p
    assert L.sb_summary(None, None, None, None) == 1
    assert L.sb_summary(None, ctypes.byref(o), ctypes.cast(row, vp), ctypes.cast(counts, vp)) == 1
    assert L.sb_summary_device(None, None, None, None) == 1
    assert L.sb_summary_device(None, ctypes.byref(o), ctypes.cast(row, vp), None) == 1


@pytest.fixture(scope="module")
def runs(sb, oracle):
    """every case on the oracle, under warnings-as-errors"""
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for c in sc.all_cases(sb):
            out[c["name"] + " mode %d" % c["mode"]] = (c,) + sc.expected(oracle, c)
    return out


def test_every_program_runs_and_compares_where_it_says(runs):
    for name, (c, exp, _) in runs.items():
        assert sorted(exp) == sorted(c["compare_after"]), name
        for k, (row, counts) in exp.items():
            assert row.shape == (24,) and row[20] == 1.0 and not row[21:].any(), (name, k)
            assert list(counts[:6]) == [int(x) for x in row[:6]], (name, k)


def test_default_scene_has_skipped_levels(runs):
    c = runs["default 120/300 mode 1"][0]
    assert (c["buf"].particle_count, c["buf"].beam_count) == (119, 299)
    assert sr.pow2_at_least(c["buf"].max_particles) == 128 and sr.pow2_at_least(c["buf"].max_beams) == 512


def test_tree_order_witness_bites(sb, runs):
    c, exp, _ = runs["tree order mode 0"]
    vx = np.zeros(4)
    vx[:3] = c["buf"].particles[:3, 2]
    assert sr.tree_sum(vx) == 1.0
    serial = 0.0
    for v in vx:
        serial += v
    assert serial == 0.0
    assert exp[-1][0][word(sb, "mean_vx")] == np.float32(1.0 / 3.0)
    neg = runs["all -0.0 mode 0"][1][-1][0][word(sb, "mean_vx")]
    pos = runs["-0.0 beside empty leaves mode 0"][1][-1][0][word(sb, "mean_vx")]
    assert neg.view(np.uint32) == 0x80000000 and pos.view(np.uint32) == 0


def test_nonfinite_case_bites(sb, runs):
    row = runs["non-finite mode 0"][1][2][0]
    assert row[word(sb, "nonfinite_particles")] >= 2 and row[word(sb, "nonfinite_beams")] > 0
    assert np.isfinite(row[6:20]).all()


def test_breaking_case_bites(sb, runs):
    exp = runs["breaking lattice mode 0"][1]
    pend, rem = word(sb, "pending_breaks"), word(sb, "removed_beams")
    assert exp[0][0][pend] > 0 and exp[0][0][rem] == 0           # mid-frame
    assert exp[1][0][pend] == 0 and exp[1][0][rem] > 0           # after the delete pass
    assert exp[1][0][rem] == exp[0][0][pend]
    assert exp[2][0][rem] >= exp[1][0][rem]


def test_permuted_case_is_not_the_identity(runs):
    buf = runs["8x6 in 5000/70000 mode 0"][0]["buf"]
    P, B, maxP = buf.particle_count, buf.beam_count, buf.max_particles
    assert not np.array_equal(buf.mapping[:P], np.arange(P)) and not np.array_equal(buf.mapping[maxP:maxP + B], np.arange(B))
    assert buf.mapping[:P].max() < 200 and buf.mapping[maxP:maxP + B].max() < 400   # far below the capacity


def test_clamp_case_is_where_the_default_cut_is_the_clamp(runs):
    """W = 2^21 for both trees: the default cut is SB_SUMMARY_MAX_PARTIALS (asserted to be 262 144 above) and not W / 4; at every
    capacity of the other cases it is W / 4 or the floor of 256.  The sums round, so the order of the additions shows."""
    c, exp, _ = runs["8x6 in 2^20+1/2^20+1 mode 0"]
    buf = c["buf"]
    for cap in (buf.max_particles, buf.max_beams):
        W = sr.pow2_at_least(cap)
        assert cap == sc.CLAMP_CAPACITY and W == 1 << 21 and sc.default_partials(W) == 262144 != W // 4
    for name, (other, _, _) in runs.items():
        if other is not c:
            for cap in (other["buf"].max_particles, other["buf"].max_beams):
                W = sr.pow2_at_least(cap)
                assert W <= 131072 and sc.default_partials(W) == max(W // 4, 256), name
    P, B, maxP = buf.particle_count, buf.beam_count, buf.max_particles
    assert P == 48 and B > 100
    assert not np.array_equal(np.sort(buf.mapping[:P]), buf.mapping[:P]) and buf.mapping[:P].max() < 200
    idx = np.sort(buf.mapping[:P].astype(np.int64))
    differs = 0
    for col in (2, 3):
        leaves = np.zeros(1 << 21)
        leaves[idx] = buf.particles[idx, col].astype(np.float64)
        serial = 0.0
        for v in leaves[idx]:
            serial += v
        differs += sr.tree_sum(leaves) != serial
    assert differs > 0
    assert sorted(exp) == [-1, 0] and exp[-1][0].tobytes() != exp[0][0].tobytes()


def test_multi_leaf_case_tree_sum_differs_from_a_flat_sum(runs):
    buf = runs["96x96 lattice mode 0"][0]["buf"]   # (as uploaded: the first comparison of the case)
    P = buf.particle_count
    assert np.array_equal(buf.mapping[:P], np.arange(P))
    differs = 0
    for col in range(4):
        leaves = np.zeros(sr.pow2_at_least(buf.max_particles))
        leaves[:P] = buf.particles[:P, col].astype(np.float64)
        differs += sr.tree_sum(leaves) != np.sum(leaves) or sr.tree_sum(leaves) != float(sum(leaves.tolist()))
    assert differs > 0


def test_no_kernel_of_the_summary_spills_or_uses_scratch():
    """the compiler's own report (tools/kernel_resources.py) for every kernel of sb_summary.hip, and the committed table is that report"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                        os.path.join(ROOT, "softbody-webgpu_amd", "csrc", "sb_summary.hip"), "k_summary"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    rows = [ln.split() for ln in p.stdout.splitlines() if "k_summary" in ln]
    names = " ".join(" ".join(r) for r in rows)
    for k in ("k_summary_init", "k_summary_row", "k_summary_fold<64>", "k_summary_particles<16>", "k_summary_beams<16>"):
        assert k in names, k
    assert len(rows) == 19
    for r in rows:
        assert r[r.index("spill") + 1] == "0" and r[r.index("scratch") + 1] == "0", r
        assert int(r[r.index("VGPR") + 1]) <= 256, r
    assert p.stdout == open(os.path.join(ROOT, "profiles", "summary_kernel_resources.txt")).read()
