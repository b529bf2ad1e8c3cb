"""sb_forces_device / sb_forces without a GPU: declared, exported, bound; the numpy restatement (tests/forces_ref.py) equals the
batch's on every scene of tests/batch_forces_cases.py and tells the batch's three wrong variants and a fourth of its own apart --
partners summed in ascending DATA-index order instead of mapping-slot order; the two new planes of the scene tables
(csrc/sb_report_tables.h) against brute force under sanitizers (tests/forces_tables_check.cpp)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_forces_cases as bfc  # noqa: E402
import batch_forces_ref as bfr  # noqa: E402
import forces_cases as fc  # noqa: E402
import forces_ref as fr  # noqa: E402
from test_hostcheck_cpu import CSRC, ENV  # noqa: E402

u4 = fr.words


# ---------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_the_calls(sb):
    names = sb.engine.declared_symbols()
    L = sb.engine.load_library()
    vp = ctypes.c_void_p
    opt = ctypes.POINTER(sb.engine.SbForcesOptions)
    for f in ("sb_forces_device", "sb_forces"):
        assert f in names and hasattr(L, f)
        assert getattr(L, f).restype is ctypes.c_int and getattr(L, f).argtypes == [vp, opt, vp, vp, vp, vp, vp]
    assert L.sb_abi_version() == 1   # additions only
    assert ctypes.sizeof(sb.engine.SbForcesOptions) == 32
    header = open(sb.engine.HEADER_PATH).read()
    for needle in ("#define SB_FORCE_WORDS 8u", "#define SB_FORCE_COUNT_WORDS 4u", "#define SB_FORCES_OTHER_BODY 1u", "forces_table_build_us",
                   "sb_forces_device only ENQUEUES", "ASCENDING MAPPING-SLOT ORDER"):
        assert needle in header, needle


def test_python_has_the_calls_and_the_batchs_names(sb):
    e = sb.engine
    assert callable(sb.Engine.forces) and callable(sb.Engine.forces_host)
    assert e.FORCE_WORDS == fr.WORDS == len(sb.batch.FORCE_FIELDS) and e.FORCE_COUNT_WORDS == fr.COUNT_WORDS == len(sb.batch.FORCE_COUNT_FIELDS)
    assert e.FORCE_FIELDS is sb.batch.FORCE_FIELDS and e.FORCE_COUNT_FIELDS is sb.batch.FORCE_COUNT_FIELDS and e.Forces is sb.batch.Forces
    assert e.FORCES_OTHER_BODY == 1


def test_a_null_handle_is_refused_before_any_device(sb):
    L = sb.engine.load_library()
    word = (ctypes.c_int64 * 64)()
    p = ctypes.cast(word, ctypes.c_void_p)
    assert L.sb_forces_device(None, None, None, p, p, p, p) == 1 and L.sb_forces(None, None, None, p, p, p, p) == 1


# ---------------------------------------------------------------- the restatement
def all_batch_scenes(sb):
    cases = [bfc.case_small(sb), bfc.case_beams(sb), bfc.case_contacts(sb), bfc.case_contacts(sb, 100), bfc.case_rings(sb), bfc.case_two_bodies(sb),
             bfc.case_mixed(sb), bfc.case_materials(sb, bfc.MATERIAL_CAPS[0])] + [bfc.case_anchor(sb, n) for n in bfc.anchor_scenes(sb)]
    return [(c, b) for c in cases for b in c["bufs"] if b is not None]


def test_equals_the_batch_reference_on_every_scene_of_its_cases(sb):
    scenes = all_batch_scenes(sb)
    assert len(scenes) >= 40
    for case, buf in scenes:
        kw = dict(radius=case.get("radius", 10.0), subticks=case.get("subticks", 64))
        got, exp = fr.forces_ref(buf, **kw), bfr.forces_ref(buf, **kw)
        assert got[3].dtype == np.int64 and got[3].tolist() == exp[3].tolist()
        assert all(np.array_equal(u4(g), u4(e)) and g.dtype == e.dtype for g, e in zip(got[:3], exp[:3])), case["name"]


def test_the_batchs_three_wrong_variants_are_told_apart(sb):
    zoo, star, kinds = bfc.contact_zoo(sb), bfc.star(sb, 1e9), bfc.beam_kinds(sb)
    assert not np.array_equal(u4(fr.forces_ref(zoo)[0]), u4(fr.forces_ref(zoo, descending=True)[0]))
    assert not np.array_equal(fr.forces_ref(star)[1], fr.forces_ref(star, saturate=False)[1])
    good, bad = fr.forces_ref(kinds), fr.forces_ref(kinds, skip_slots=(0,))
    assert good[3].tolist() == [6, 3, 0, 0] and bad[3].tolist() == [6, 2, 0, 0] and not np.array_equal(u4(good[2]), u4(bad[2]))


def test_data_index_order_differs_on_the_permuted_five(sb):
    """the mapping-order case: a non-trivial permutation, a particle with five partners, sums whose bits depend on the order"""
    buf = fc.permuted_five(sb)
    P = buf.particle_count
    d = buf.mapping[:P].astype(int)
    assert d[:6].tolist() == list(fc.PERMUTED) and sorted(d.tolist()) != d.tolist() and len(set(d.tolist())) == P
    by_slot, by_data = fr.forces_ref(buf), fr.forces_ref(buf, by_data_index=True)
    centre = d[0]
    assert by_slot[0][centre, 7] == 5.0 == by_data[0][centre, 7]
    order = np.argsort(d[1:6])                 # the partners' slots in ascending data-index order: 3, 1, 5, 2, 4
    assert (order + 1).tolist() == [3, 1, 5, 2, 4]
    assert (u4(by_slot[0][centre, 2:6]) != u4(by_data[0][centre, 2:6])).any(), "the two orders give the same bits: the case does not bite"
    # everything that does not depend on the order is the same: depth, partners, the beams, the counts
    assert np.array_equal(u4(by_slot[0][:, 6:]), u4(by_data[0][:, 6:])) and by_slot[3].tolist() == by_data[3].tolist()
    # and on a scene whose mapping is the identity the fourth variant is no variant
    ident = bfc.crowded_cell(sb)
    assert np.array_equal(u4(fr.forces_ref(ident)[0]), u4(fr.forces_ref(ident, by_data_index=True)[0]))


def test_the_engine_cases_hold_what_they_promise(sb):
    for n in (63, 64, 65, 257):
        buf = fc.beam_chain(sb, n)
        out = fr.forces_ref(buf)
        assert out[3].tolist() == [n + 1, n, 0, 0] and (out[2][:n] != 0).all() and not out[2][n:].any()
    gate = fc.beam_chain(sb, 257, gate=True)
    out = fr.forces_ref(gate)
    with np.errstate(invalid="ignore"):
        assert out[3][3] == 0 and (np.abs(out[2]) > 1e15).sum() >= 30      # far endpoints: huge, finite tensions
    P = gate.particle_count
    pos = gate.particles[gate.mapping[:P].astype(int), :2]
    rec = gate.beams[:257]
    dx = gate.particles[rec["b"].astype(int), :2] - gate.particles[rec["a"].astype(int), :2]
    len2 = (dx.astype(np.float64) ** 2).sum(axis=1)
    inside = (len2 >= 2.0 ** -90) & (len2 <= 2.0 ** 90)
    for w in range(0, 256, 64):                 # every full wave of 64 caller slots mixes beams inside and outside the gate
        assert inside[w:w + 64].any() and (~inside[w:w + 64]).any()
    assert (len2 == 0).sum() >= 20 and np.isfinite(pos).all()
    names = [n for n, _, _ in fc.engine_scenes(sb)]
    assert len(names) >= 30 and len(set(names)) == len(names)


# ---------------------------------------------------------------- the new table builders under sanitizers
@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_table_builders_under_sanitizers(san):
    target = os.path.join("hostcheck_build", "forces_tables_check_" + san)
    p = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    for P, B in ((1000, 3000), (4000, 300000)):      # (the second: several host threads a plane)
        r = subprocess.run([os.path.join(CSRC, target), str(P), str(B)], capture_output=True, text=True, timeout=300, env=ENV)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr, r.stderr[-4000:]
        assert "FORCES_TABLES_OK %d particles %d beams 5 defects" % (P, B) in r.stdout, r.stdout
