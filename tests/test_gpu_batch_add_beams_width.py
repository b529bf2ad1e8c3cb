"""BatchEngine.add_beams (k_batch_add_beams, sb_batch_add.hip) at the widths its code is written for: 64 rows, up to
three flag words, 128 bitmap words, capacities that are no multiple of 4 or 32.  tests/test_gpu_batch_add_beams.py stops at 16 rows
and 320 beams.  Every comparison is bit for bit through its check_against_ref (result, counts, the edited scene as load_scene
returns it); the frames after equal the oracle started from the restatement's edit.  tests/test_batch_add_beams_cpu.py asserts on
the restatement alone that each case of tests/batch_add_beams_cases.py is what it is named for."""
import numpy as np
import pytest

import batch_add_beams_cases as cases
import batch_add_beams_ref as ref
import batch_bodies_ref
import graph_ref
from batch_harness import load_all
from test_gpu_batch_add_beams import GRID, OFF, ALLPAIRS, add, batch, check_against_ref, dev, oracle_frames, raw
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


def summary(be, scene=0):
    """(beams, removed, pending) of a scene"""
    return be.summary().cpu().numpy()[scene, [1, 2, 3]].tolist()


def oracle_with_bits(oracle, buf, slots, mode=OFF):
    """one frame of the oracle from `buf` with the delete bits of `slots` set"""
    r = oracle.OracleEngine(1000.0, 10.0, 64, buf.layout, mode, threads=4)
    r.write_buffers(buf)
    for s in slots:
        bit = buf.max_particles + int(s)
        r.delete[bit >> 5] |= np.uint32(1 << (bit & 31))
    r.frame()
    return r.load_buffers(buf.copy())


@pytest.mark.parametrize("name", list(cases.FLAG_WORD_CASES))
def test_pending_bits_of_the_new_slots(sb, oracle, name):
    """"The pending bits of the new slots (at most three flag words)": 64 rows onto 30 beams clear bits 30 .. 31 of word 0, the whole
    of word 1 (lo = 0, hi = 31) and bits 0 .. 29 of word 2; 32 rows onto 32 beams one whole word; 2 rows onto 31 beams bit 31 of
    word 0 and bit 0 of word 1.  The flags of the two slots in front (raised by a cut, in the same first word in two of the cases)
    survive the clear: the next frame removes exactly those two and keeps every new beam.  With 64 rows this is also the full
    width of the candidate ballot, (1ull << tid) - 1 at tid == 63 included."""
    case = cases.flag_words_case(sb, name)
    bc, k = cases.FLAG_WORD_CASES[name]
    be = batch(sb, case)
    hit, c = be.cut(dev(case["cut"]), hit=True)
    cut_idx = case["bufs"][0].mapping[32 + bc - 2:32 + bc].astype(np.int64)
    assert c.cpu().numpy().tolist() == [[bc, 2, 2, 0]] and sorted(hit.cpu().numpy()[0].nonzero()[0].tolist()) == sorted(cut_idx.tolist())
    after, res, cnt = check_against_ref(be, case, case["flags"], what=name)
    assert cnt == [[k, 0, 0, 0]] and summary(be) == [float(bc + k), 0.0, 2.0], "2 pending, Bc + k beams"
    be.frame()
    got = be.load_scene(0, after[0].copy())
    alive = ref.alive_set(got)
    assert got.beam_count == bc + k - 2 and alive[res[0]].all() and not alive[cut_idx].any(), "exactly the two cut beams go"
    assert_same(got, oracle_with_bits(oracle, after[0], case["cut_slots"]), name + ": the frame after == the oracle with the same two delete bits")
    assert summary(be) == [float(bc + k - 2), 2.0, 0.0]
    be.destroy()


def test_rows_32_to_63_under_skip_joined(sb, oracle):
    """Rows 32 to 63: the second word of s_joined (rows 33, 47 and 63 / 61 name pairs a live beam joins, one with its endpoints
    swapped), the in-call duplicate scan across the row-32 boundary (row 40 repeats row 3, row 62 repeats row 35), and the upper
    half of the 64-bit candidate ballot, with an INVALID and an EMPTY row going round rows 31, 32 and 63 in the three scenes so
    that the ranks behind them shift across the half boundary."""
    case = cases.upper_half_case(sb)
    be = batch(sb, case)
    after, res, cnt = check_against_ref(be, case, case["flags"], what="upper half")
    for s in range(3):
        assert [j for j in range(64) if res[s][j] == ref.JOINED] == case["joined_rows"][s], s
        assert res[s][cases.UPPER_SPECIAL[s]] == ref.INVALID and res[s][cases.UPPER_SPECIAL[(s + 1) % 3]] == ref.EMPTY
    assert all(res[0][j] == ref.JOINED for j in (33, 47, 63, 40, 62))
    assert cnt == [[57, 1, 5, 0]] * 3
    be.frame()
    for s, got in enumerate(load_all(be, after)):
        assert_same(got, oracle_frames(oracle, after[s], 1, OFF), "scene %d: the frame after == oracle" % s)
    be.destroy()


def test_capacity_1024_4096(sb, oracle):
    """The free-index search at 4096 beams (128 bitmap words): (a) the 40 free indices lie above 4000, so the binary search lands in
    the last three words and the bit-clear loop runs up to fifteen times inside one word; 24 rows are FULL.  (b) a full scene: 64 x
    FULL and no byte changes.  (c) the SKIP_JOINED sweep over 700 live beams takes three trips of the 256-thread loop, and the beams
    that join the named pairs sit in slots above 512, the third trip.  graph(adjacency=True) and bodies() after the add equal their
    restatements on the edited scenes; four substeps after equal the oracle."""
    import torch
    case = cases.big_case(sb)
    be = batch(sb, case, GRID)
    full_before = [x[1].cpu().numpy().tobytes() for x in be.state_tensors()] + [be.summary()[1].cpu().numpy().tobytes()]
    after, res, cnt = check_against_ref(be, case, case["flags"], what="1024 / 4096")
    F_ = ref.FULL
    assert res[0].tolist() == cases.BIG_FREE + [F_] * 24 and res[1].tolist() == [F_] * 64
    assert [j for j in range(64) if res[2][j] == ref.JOINED] == case["joined_rows"]
    assert cnt == [[40, 0, 0, 24], [0, 0, 0, 64], [48, 0, 16, 0]]
    assert [x[1].cpu().numpy().tobytes() for x in be.state_tensors()] + [be.summary()[1].cpu().numpy().tobytes()] == full_before, "(b): no byte changes"
    assert_same(after[1], case["bufs"][1], "(b) as uploaded")
    want = graph_ref.graph_of(after, *cases.BIG_CAP)
    got = graph_ref.Graph(*(x.cpu().numpy() for x in be.graph(ends=True, material=True, adjacency=True)))
    assert graph_ref.same(got, want) == []
    labels, counts = (x.cpu().numpy() for x in be.bodies())
    wl, _, wc = batch_bodies_ref.bodies_of(after, cases.BIG_CAP[0])
    assert np.array_equal(labels, wl) and np.array_equal(counts, wc)
    be.step(4)
    for s, got in enumerate(load_all(be, after)):
        r = oracle.OracleEngine(1000.0, 10.0, 64, 2, ALLPAIRS, threads=4)
        r.write_buffers(after[s])
        r.step(4)
        assert_same(got, r.load_buffers(after[s].copy()), "scene %d: four substeps after == oracle" % s)
    be.destroy()


def test_free_slots_but_no_free_index(sb, oracle):
    """FULL because r >= n_free while Bc + r < max_beams: three of 40 beams are cut and removed by a frame, so three slots are free,
    but every data index is alive in the current or in the reset state.  After a checkpoint the same rows get the three removed
    indices in ascending order."""
    case = cases.no_index_case(sb)
    buf = case["bufs"][0]
    be = batch(sb, case)
    _, c = be.cut(dev(case["cut"]))
    assert c.cpu().numpy().tolist() == [[40, 3, 3, 0]]
    be.frame()
    assert summary(be) == [37.0, 3.0, 0.0]
    now = load_all(be, case["bufs"])
    _, res, cnt = check_against_ref(be, case, 0, before=now, reset_alive=[ref.alive_set(buf)], what="no free index")
    assert res[0].tolist() == [ref.FULL] * 3 and cnt == [[0, 0, 0, 3]] and now[0].beam_count + 3 <= be.max_beams
    be.checkpoint()
    after, res, cnt = check_against_ref(be, case, 0, before=now, reset_alive=[ref.alive_set(now[0])], what="after a checkpoint")
    assert res[0].tolist() == sorted(case["cut_slots"]) and cnt == [[3, 0, 0, 0]] and summary(be) == [40.0, 0.0, 0.0]
    be.frame()
    assert_same(be.load_scene(0, after[0].copy()), oracle_frames(oracle, after[0], 1, OFF), "the frame after == oracle")
    be.destroy()


@pytest.mark.parametrize("cap", cases.ODD_CAPS, ids=lambda c: "%d-%d" % c)
def test_odd_capacities(sb, oracle, cap):
    """Capacities that are no multiple of 4 or 32 beams and an odd max_particles: the alive bytes are read four to a load under the
    guard d0 + e < maxB, the last bitmap word is partial, and the inverse table's last word holds one particle (the one at data
    index max_particles - 1, which every row joins).  The last free index, max_beams - 1, is taken and two more rows are FULL.
    The scenes before and behind in the batch, and every state row the add does not name, stay as in a batch that never added."""
    case = cases.odd_case(sb, cap)
    be, plain = batch(sb, case), batch(sb, case)
    after, res, cnt = check_against_ref(be, case, case["flags"], what="odd %d / %d" % cap)
    added = res[1][res[1] >= 0]
    assert added[-1] == cap[1] - 1 and res[1][-2:].tolist() == [ref.FULL] * 2 and cnt == [[0, 0, 0, 0], [cases.ODD_FREE, 0, 0, 2], [0, 0, 0, 0]]
    keep = np.ones(cap[1], bool)
    keep[added] = False
    for name, x, y in zip(("particles", "beams", "alive"), be.state_tensors(), plain.state_tensors()):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert x[[0, 2]].tobytes() == y[[0, 2]].tobytes(), name + ": the neighbouring scenes"
        assert (x[1] if name == "particles" else x[1][keep]).tobytes() == (y[1] if name == "particles" else y[1][keep]).tobytes(), name
    assert be.state_tensors()[2].cpu().numpy()[1][added].all()
    for x in (be, plain):
        x.frame()
    got, unc = load_all(be, after), load_all(plain, case["bufs"])
    assert_same(got[1], oracle_frames(oracle, after[1], 1, OFF), "the frame after == oracle")
    for s in (0, 2):
        assert_same(got[s], unc[s], "scene %d == never added" % s)
    be.destroy()
    plain.destroy()
