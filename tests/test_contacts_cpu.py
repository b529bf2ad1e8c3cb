"""Engine.contacts() (sb_contacts / sb_contacts_device) without a GPU: the header declares the calls, the library
exports them, engine.py binds them with a structure of the C struct's size, a NULL handle is refused before anything touches a
device, the row-chunked reference equals the batch's on every scene of the batch's cases and a scene worked out by hand, every
scene of tests/test_gpu_contacts.py BITES on the reference alone -- the two scenes past 256 scan blocks against a model of the scan
whose loop over the block sums drops its carry --, the reference's pruning changes no output, and no kernel of the call spills or
uses scratch."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_contacts_ref as cr  # noqa: E402
import contacts_cases as cc  # noqa: E402
import contacts_ref as cref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sb_contacts", "sb_contacts_device"]


def test_header_declares_and_library_exports_the_calls(sb):
    names = sb.engine.declared_symbols()
    L = sb.engine.load_library()
    for s in SYMBOLS:
        assert s in names, s
        assert hasattr(L, s), s
    assert L.sb_abi_version() == 1   # additions only
    vp, po = ctypes.c_void_p, ctypes.POINTER(sb.engine.SbContactsOptions)
    assert L.sb_contacts_device.argtypes == [vp, po, vp, vp, vp, vp] and L.sb_contacts.argtypes == [vp, po, vp, vp, vp, vp]
    assert callable(sb.Engine.contacts) and callable(sb.Engine.contacts_host)


def test_options_structure_and_words_are_the_c_headers(sb, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "softbody.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %u %u %u %u %u\\n", sizeof(sb_contacts_options), offsetof(sb_contacts_options, flags), '
                   'offsetof(sb_contacts_options, max_pairs), offsetof(sb_contacts_options, reserved), SB_CONTACT_WORDS, '
                   'SB_CONTACT_COUNT_WORDS, SB_BATCH_CONTACT_WORDS, SB_CONTACTS_OTHER_BODY, SB_BATCH_CONTACTS_OTHER_BODY); return 0; }\n')
    exe = str(tmp_path / "size")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    size, o_flags, o_pairs, o_reserved, words, cwords, bwords, flag, bflag = (int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split())
    O = sb.engine.SbContactsOptions
    assert ctypes.sizeof(O) == size == 32 and (O.flags.offset, O.max_pairs.offset, O.reserved.offset) == (o_flags, o_pairs, o_reserved) == (4, 8, 16)
    assert words == bwords == sb.engine.CONTACT_WORDS == len(sb.engine.CONTACT_TOUCH_FIELDS) == cref.WORDS
    assert cwords == sb.engine.CONTACT_COUNT_WORDS == len(sb.engine.CONTACT_COUNT_FIELDS)
    assert flag == bflag == sb.engine.CONTACTS_OTHER_BODY


def test_field_names_are_the_batchs_not_a_copy(sb):
    assert sb.engine.CONTACT_TOUCH_FIELDS is sb.batch.CONTACT_TOUCH_FIELDS and sb.engine.CONTACT_COUNT_FIELDS is sb.batch.CONTACT_COUNT_FIELDS
    assert (sb.engine.WALL_LEFT, sb.engine.WALL_RIGHT, sb.engine.WALL_LOW, sb.engine.WALL_HIGH) == (cr.LEFT, cr.RIGHT, cr.LOW, cr.HIGH)


def test_null_handle_is_invalid_before_anything_touches_a_device(sb):
    L = sb.engine.load_library()
    touch, counts = (ctypes.c_int32 * 32)(), (ctypes.c_int64 * 4)()
    o = sb.engine.SbContactsOptions()
    o.struct_size = ctypes.sizeof(o)
    vp = ctypes.c_void_p
    assert L.sb_contacts(None, None, None, None, None, None) == 1
    assert L.sb_contacts(None, ctypes.byref(o), None, ctypes.cast(touch, vp), None, ctypes.cast(counts, vp)) == 1
    assert L.sb_contacts_device(None, None, None, None, None, None) == 1
    assert L.sb_contacts_device(None, ctypes.byref(o), None, ctypes.cast(touch, vp), None, None) == 1


def test_reference_on_a_scene_worked_out_by_hand(sb):
    """radius 10, bounds 100.  Particles (number: data index, position): 0: 7 (10, 50) on the left wall; 1: 2 (29.5, 50) touches 0
    (19.5 apart); 2: 5 (49.5, 50) exactly 20 from 1: no contact; 3: 0 (49.5, 50) on the same spot as 2 (dist 0: contact), so it is
    20 from 1 as well; 4: 3 (90, 90) in the far corner, alone.  Pairs by data index: (0, 5), (2, 7)."""
    buf = sb.Buffers(2, 8, 4)
    D = [7, 2, 5, 0, 3]
    buf.particles[D, :2] = np.array([(10.0, 50.0), (29.5, 50.0), (49.5, 50.0), (49.5, 50.0), (90.0, 90.0)], "f4")
    buf.mapping[:5] = [3, 7, 0, 5, 2]
    buf.particle_count = 5
    labels = np.array([1, 9, 4, 9, 9, 1, 9, 4], np.int32)      # 0 and 5 one body, 2 and 7 another
    touch, pairs, counts = cref.contacts_ref(buf, 10.0, 100.0, labels, 3)
    assert counts.dtype == np.int64 and counts.tolist() == [2, 0, 2, 4]
    assert pairs.tolist() == [[0, 5], [2, 7], [-1, -1]]
    rows = {0: [1, 0, 0, 5], 5: [1, 0, 0, 0], 2: [1, 0, 0, 7], 7: [1, 0, cr.LEFT, 2], 3: [0, 0, cr.RIGHT | cr.HIGH, -1]}
    for d in range(8):
        assert touch[d].tolist() == rows.get(d, [0, 0, 0, -1]), d
    labels[5] = 2
    touch, pairs, counts = cref.contacts_ref(buf, 10.0, 100.0, labels, 3, other_body=True)
    assert counts.tolist() == [2, 1, 2, 4] and pairs.tolist() == [[0, 5], [-1, -1], [-1, -1]] and touch[0].tolist() == [1, 1, 0, 5]
    touch, pairs, counts = cref.contacts_ref(buf, 10.0, 100.0, None, 1)
    assert counts.tolist() == [2, -1, 2, 4] and pairs.tolist() == [[0, 5]] and touch[4].tolist() == [0, -1, 0, -1]


def test_chunked_reference_equals_the_batchs_on_every_scene_of_its_cases(sb):
    scenes = cc.batch_scenes(sb)
    assert len(scenes) >= 30 and sum(not s["finite"] for s in scenes) >= 2
    for s in scenes:
        lab = cc.striped_labels(s["buf"].max_particles)
        for labels, m, other in ((None, 0, False), (None, 40, False), (lab, 40, False), (lab, 40, True)):
            a = cref.contacts_ref(s["buf"], s["radius"], s["bounds"], labels, m, other)
            b = cr.contacts_ref(s["buf"], s["radius"], s["bounds"], labels, m, other)
            assert a[2].dtype == np.int64 and b[2].dtype == np.int32
            for x, y in zip(a, b):
                assert np.array_equal(x, y), (s["name"], m, other)


# name: (cells per side, counts with striped labels) -- the counts as the reference gives them on the CPU
BITES = {"pile 4097 in 5000": (98, (3992, 3197, 0, 3956)), "box 16384": (295, (16099, 12829, 0, 15869)),
         "32 cells per side": (32, (139, 109, 1, 129)), "64 cells per side": (64, (353, 298, 8, 352)),
         "crowd 600": (49, (178607, 143114, 0, 600))}


@pytest.mark.parametrize("name", list(cc.BIG))
def test_scene_is_what_its_construction_says(sb, name):
    s = cc.big_scene(sb, name)
    buf, D = s["buf"], s["D"]
    P, maxP = buf.particle_count, buf.max_particles
    touch, _, counts = cc.expected(s, cc.striped_labels(maxP), key="striped")
    cells, exp = BITES[name]
    assert tuple(counts.tolist()) == exp and cc.cells_per_side(s["bounds"], s["radius"], P) == cells
    assert not np.array_equal(D, np.arange(P)) and not np.array_equal(np.sort(buf.mapping[:P]), buf.mapping[:P])
    assert (touch[:, 0] > 0).sum() == counts[3] and touch[:, 0].sum() == 2 * counts[0] and 0 < counts[1] < counts[0]
    pairs = cc.expected(s, None, int(counts[0]), key="all")[1]
    if name.startswith("pile"):
        assert P == 4097 > 4096 and maxP == 5000
        for edge in (256, 4096):     # pairs straddle the workgroup and the scan-block boundaries of the data indices
            assert ((pairs[:, 0] < edge) & (pairs[:, 1] >= edge)).any(), edge
    if name.startswith("box"):
        assert (cells * cells + 1) > 80 * cc.SCAN_BLOCK
    if "cells per side" in name:
        assert (cells * cells) % cc.SCAN_BLOCK == 0      # the count words are one more than whole blocks
    if name.startswith("crowd"):
        f = np.float32
        cell = f(1000.0) / f(49)
        x = buf.particles[D, :2]
        assert len(np.unique((x / cell).astype(int), axis=0)) == 1 and touch[:, 0].max() > 500
        above = np.bincount(pairs[:, 0], minlength=maxP)
        assert above.max() > 400         # far more than the four partners a list sweep keeps


def test_scan_model_is_the_exclusive_scan():
    rng = np.random.default_rng(3)
    for n in (1, 1023, 1024, 1025, cc.SECOND_TRIP, cc.SECOND_TRIP + 1, cc.SECOND_TRIP + 2 * cc.SCAN_BLOCK + 7):
        w = rng.integers(0, 5, n)
        out, total = cc.scan_model(w)
        assert np.array_equal(out, np.cumsum(w) - w) and total == w.sum(), n
        wrong = cc.scan_model(w, carry=False)[0]
        assert np.array_equal(wrong[:cc.SECOND_TRIP], out[:cc.SECOND_TRIP])
        assert n <= cc.SECOND_TRIP or np.array_equal(wrong[cc.SECOND_TRIP:], out[cc.SECOND_TRIP:] - w[:cc.SECOND_TRIP].sum())


def test_pruned_reference_equals_the_unpruned_on_every_existing_scene(sb):
    """contacts_ref(prune=True) is what only the scene of 40 000 particles is compared with; here against prune=False, every output"""
    def same(a, b, what):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y), what
    scenes = cc.batch_scenes(sb)
    assert sum(not s["finite"] for s in scenes) >= 2        # coordinates that are not finite among them
    for s in scenes:
        lab = cc.striped_labels(s["buf"].max_particles)
        for labels, m, other in ((None, 0, False), (None, 40, False), (lab, 40, False), (lab, 40, True)):
            same(cref.contacts_ref(s["buf"], s["radius"], s["bounds"], labels, m, other, prune=True),
                 cref.contacts_ref(s["buf"], s["radius"], s["bounds"], labels, m, other), (s["name"], m, other))
    for name in cc.BIG:
        s = cc.big_scene(sb, name)
        assert not s.get("prune")
        lab = cc.striped_labels(s["buf"].max_particles)
        total = int(cc.expected(s, lab, key="striped")[2][0])
        same(cref.contacts_ref(s["buf"], s["radius"], s["bounds"], lab, prune=True), cc.expected(s, lab, key="striped"), name)
        same(cref.contacts_ref(s["buf"], s["radius"], s["bounds"], None, total, prune=True), cc.expected(s, None, total, key="all"), name)
        same(cref.contacts_ref(s["buf"], s["radius"], s["bounds"], lab, 50, True, prune=True),
             cc.expected(s, lab, 50, True, key="other 50"), name)


# name: (cells per side, blocks of the cell scan, blocks of the scan over the data indices, counts with striped labels)
PAST_FIGURES = {"544 cells per side": (544, 290, 40, (29338, 23426, 99, 27549)), "indices past 2^18": (83, 7, 260, (5904, 4721, 0, 5805))}


@pytest.mark.parametrize("name", list(cc.PAST))
def test_scene_reaches_the_second_trip_of_the_scan_of_the_block_sums(sb, name):
    """From the reference and the constants alone: more than 256 scan blocks, a nonzero carry into the second trip, touching pairs
    on both sides of it, and a scan that leaves the carry out is wrong at words the outputs are read through."""
    s = cc.big_scene(sb, name)
    buf, D = s["buf"], s["D"]
    P, maxP, edge = buf.particle_count, buf.max_particles, cc.SECOND_TRIP
    cells, cell_blocks, index_blocks, exp = PAST_FIGURES[name]
    touch, _, counts = cc.expected(s, cc.striped_labels(maxP), key="striped")
    G, word = cc.cell_words(s)
    blocks = lambda n: (n + cc.SCAN_BLOCK - 1) // cc.SCAN_BLOCK
    assert tuple(counts.tolist()) == exp and G == cells == cc.cells_per_side(s["bounds"], s["radius"], P)
    assert (blocks(G * G + 1), blocks(int(D.max()) + 1)) == (cell_blocks, index_blocks)
    assert not np.array_equal(D, np.arange(P)) and not np.array_equal(np.sort(buf.mapping[:P]), buf.mapping[:P])
    assert (touch[:, 0] > 0).sum() == counts[3] and touch[:, 0].sum() == 2 * counts[0] and 0 < counts[1] < counts[0]
    above, total = cc.pairs_above(s)
    pairs = cc.expected(s, None, total, key="all")[1]
    assert total == counts[0] == above.sum()
    if name.startswith("544"):
        assert s["prune"] and P == 40000 and G >= 530 and G * G <= 8 * P and cell_blocks > cc.SCAN_SUMS >= index_blocks
        words = np.bincount(word, minlength=G * G + 1)          # what k_contacts_bin leaves: a count per cell, and the word behind
        carry = int(words[:edge].sum())
        assert 0 < carry < P and carry == (word < edge).sum()
        assert word.min() < G and word.max() == G * G - 1 and words[-1] == 0       # the first row and the last cell are lived in
        at = np.zeros(maxP, np.int64)
        at[D] = word
        a, b = at[pairs[:, 0]], at[pairs[:, 1]]
        assert ((a < edge) & (b < edge)).any() and ((a >= edge) & (b >= edge)).any() and ((a < edge) != (b < edge)).sum() > 100
        used = words > 0        # a cell's start is read for every cell somebody lives in (and its end is the next start)
    else:
        assert maxP == edge + 4096 and index_blocks > cc.SCAN_SUMS >= cell_blocks
        words = above                                           # what k_contacts_visit leaves: pairs listed under every data index
        carry = int(words[:edge].sum())
        assert 0 < carry < total
        assert (pairs[:, 0] < edge).sum() > 1000 and (pairs[:, 0] >= edge).sum() > 1000
        assert ((pairs[:, 0] < edge) & (pairs[:, 1] >= edge)).any()
        used = words > 0        # a particle reads its place iff pairs are listed under it
    cut = cc.cut_of(s)                                          # the truncating max_pairs of the GPU test
    if name.startswith("544"):
        assert 0 < cut < total
    else:                                                       # ... behind the carry: the last pair kept is the second trip's
        assert carry < cut < total and pairs[cut - 1, 0] >= edge
    right, sum_ = cc.scan_model(words)
    wrong, _ = cc.scan_model(words, carry=False)
    assert sum_ == words.sum() and np.array_equal(right, np.cumsum(words) - words)
    bad = np.flatnonzero((wrong != right) & used)
    assert bad.size > 100 and bad.min() >= edge and np.array_equal(wrong[:edge], right[:edge])
    assert (wrong[bad] == right[bad] - carry).all()


def test_no_kernel_of_the_contacts_spills_or_uses_scratch():
    """the compiler's own report (tools/kernel_resources.py) for every kernel of sb_contacts.hip and for the scan it launches
    (sb_report.hip), and the committed tables are that report"""
    csrc = os.path.join(ROOT, "softbody-webgpu_amd", "csrc")
    for src, prefix, table, kernels in (
            ("sb_contacts.hip", "k_contacts", "contacts_kernel_resources.txt",
             ("k_contacts_bin", "k_contacts_scatter", "k_contacts_visit", "k_contacts_list", "k_contacts_tail", "k_contacts_counts")),
            ("sb_report.hip", "k_report", "report_kernel_resources.txt",
             ("k_report_scan_reduce<unsigned int>", "k_report_scan_reduce<unsigned long long>", "k_report_scan_sums<unsigned int>",
              "k_report_scan_sums<unsigned long long>", "k_report_scan_add<unsigned int>", "k_report_scan_add<unsigned long long>"))):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), os.path.join(csrc, src), prefix],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        rows = [ln.split() for ln in p.stdout.splitlines() if prefix in ln]
        names = " ".join(" ".join(r) for r in rows)
        for k in kernels:
            assert k in names, k
        assert len(rows) == len(kernels) == 6
        for r in rows:
            assert r[r.index("spill") + 1] == "0" and r[r.index("scratch") + 1] == "0", r
        assert p.stdout == open(os.path.join(ROOT, "profiles", table)).read()
