"""BatchEngine.add_beams (sb_batch_add_beams_device) on the GPU, every comparison bit for bit: the edit equals
tests/batch_add_beams_ref.py on what load_scene returns; the frames after equal the oracle started from the edited scene; adding
on the device equals uploading the edited scene; every row code; room; which index and which flag word a new beam gets; reset,
checkpoint, cut and fork around an add; a dry run; contacts -> new_beam_rows -> add_beams welds two bodies into one."""
import numpy as np
import pytest

import batch_add_beams_cases as cases
import batch_add_beams_ref as ref
from batch_harness import load_all, make_batch, upload_each
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

OFF, ALLPAIRS, GRID = 0, 1, 2
LC, SJ = ref.LENGTH_CURRENT, ref.SKIP_JOINED


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def batch(sb, case, mode=OFF):
    case = dict(case, mode=mode)
    be = make_batch(sb, case, mode=mode)
    upload_each(be, case["bufs"])
    return be


def add(be, rows, flags=0, dry=False):
    res, cnt = be.add_beams(dev(rows), length_current=bool(flags & LC), skip_joined=bool(flags & SJ), dry_run=dry)
    return res.cpu().numpy(), cnt.cpu().numpy().tolist()


def raw(be):
    """every byte the reports can see: state rows, summary, bodies"""
    p, b, a = be.state_tensors()
    return [x.cpu().numpy().tobytes() for x in (p, b, a, be.summary(), *be.bodies())]


def check_against_ref(be, case, flags, before=None, reset_alive=None, what=""):
    """add_beams on `be` == the restatement on what load_scene returned before; returns (after, result, counts)"""
    before = load_all(be, case["bufs"]) if before is None else before
    want = cases.expected(case, flags, loaded=before, reset_alive=reset_alive)
    res, cnt = add(be, case["rows"], flags)
    for i, (edited, r, c) in enumerate(want):
        print(what, "scene", i, "result", res[i].tolist(), "want", r.tolist(), "counts", cnt[i], c)
    for i, (edited, r, c) in enumerate(want):
        assert res[i].tolist() == r.tolist() and cnt[i] == c, (what, i)
    after = [None if b is None else be.load_scene(i, b.copy()) for i, b in enumerate(before)]
    for i, (edited, _, _) in enumerate(want):
        if edited is not None:
            assert_same(after[i], edited, "%s: scene %d after the add == the restatement's edit" % (what, i))
    return after, res, cnt


def oracle_frames(oracle, buf, frames, mode):
    r = oracle.OracleEngine(1000.0, 10.0, 64, buf.layout, mode, threads=4)
    r.write_buffers(buf)
    for _ in range(frames):
        r.frame()
    return r.load_buffers(buf.copy())


@pytest.mark.parametrize("flags", [pytest.param(0, id="given-lengths"), pytest.param(LC | SJ, id="current-skip-joined")])
@pytest.mark.parametrize("mode", [pytest.param(OFF, id="off"), pytest.param(GRID, id="default")])
def test_restatement_then_oracle(sb, oracle, mode, flags):
    """1 and 2: eight default scenes, each with its own rows; then two frames against the oracle from the edited scenes (scene 2's
    first beam, given a tiny strain_break_limit, breaks and is removed inside them)"""
    case = cases.default_case(sb)
    be = batch(sb, case, mode)
    after, res, cnt = check_against_ref(be, case, flags, what="default")
    assert sum(c[0] for c in cnt) >= 40
    be.frame(2)
    got = load_all(be, after)
    for i, b in enumerate(after):
        assert_same(got[i], oracle_frames(oracle, b, 2, ALLPAIRS if mode else OFF), "scene %d: two frames after the add == oracle" % i)
    if not flags:
        i, j = case["breaking"]
        assert not ref.alive_set(got[i])[res[i][j]] and got[i].beam_count < after[i].beam_count, "the brittle beam broke and was removed"
    assert be.info("add_beams_kernel_vgprs") > 0 and be.info("add_beams_kernel_scratch_bytes") == 0
    be.destroy()


def test_equals_the_host_route(sb):
    """3: add_beams == write_scene of the restatement's edit: exported state, reports, and one frame later"""
    case = cases.default_case(sb)
    a, b = batch(sb, case, GRID), batch(sb, case, GRID)
    want = cases.expected(case, 0)
    add(a, case["rows"])
    upload_each(b, [w[0] for w in want])
    assert raw(a) == raw(b)
    for x in (a, b):
        x.frame()
    assert raw(a) == raw(b)
    for i, (ga, gb) in enumerate(zip(load_all(a, case["bufs"]), load_all(b, case["bufs"]))):
        assert_same(ga, gb, "scene %d: device route == host route after a frame" % i)
    a.destroy()
    b.destroy()


def test_row_codes(sb):
    """4: every code in one scene, with and without SKIP_JOINED, and under LENGTH_CURRENT; the beam (0, 1) carries a pending flag"""
    case, shapes = cases.codes_case(sb)
    E, I, J = ref.EMPTY, ref.INVALID, ref.JOINED
    for flags, codes in ((SJ, [I, I, I, I, I, I, I, I, I, 299, J, J, 300, J, E, I]), (0, [I, I, I, I, I, I, I, I, I, 299, 300, 301, 302, 303, E, I]),
                         (SJ | LC, [I, I, I, I, I, 299, 300, 301, 302, I, J, J, 303, J, E, I])):
        be = batch(sb, case)
        _, c = be.cut(dev(shapes))
        assert c.cpu().numpy().tolist() == [[299, 1, 1, 0]] and be.summary().cpu().numpy()[0, 3] == 1.0, "the beam (0, 1) alone is flagged"
        _, res, _ = check_against_ref(be, case, flags, what="codes, flags %d" % flags)
        assert res[0].tolist() == codes
        assert be.summary().cpu().numpy()[0, 3] == 1.0, "the pending flag of the cut beam stays"
        be.destroy()


def test_room(sb):
    """5: four of eight rows find room; a full scene; a scene never uploaded (all INVALID, its blobs untouched)"""
    case = cases.room_case(sb)
    be = batch(sb, case)
    before = raw(be)
    _, res, cnt = check_against_ref(be, case, 0, what="room")
    F = ref.FULL
    assert res.tolist() == [[36, 37, 38, 39, F, F, F, F], [F] * 8, [ref.INVALID] * 8] and cnt == [[4, 0, 0, 4], [0, 0, 0, 8], [0, 8, 0, 0]]
    now = raw(be)
    plain = batch(sb, case)
    for x, y in zip(be.state_tensors(), plain.state_tensors()):
        assert x[1:].cpu().numpy().tobytes() == y[1:].cpu().numpy().tobytes(), "the full and the never-uploaded scene are untouched"
    assert now != before and be.summary().cpu().numpy()[:, 1].tolist() == [40.0, 40.0, 0.0]
    be.destroy()
    plain.destroy()


def test_index_choice_and_flag_words(sb, oracle):
    """6: sparse mappings out of slot order: the r-th added beam gets the r-th smallest free index; new slots 30 .. 34 straddle a
    flag word.  The new slots' flags are raised by a cut and dropped by a reset (which takes the reset state's flag words), the add
    is repeated: the pending bits of the new slots are clear and the next frame keeps all five beams."""
    case = cases.sparse_case(sb)
    be = batch(sb, case)
    after, res, cnt = check_against_ref(be, case, 0, what="sparse")
    assert res[0].tolist() == [4, 5, 6, 11, 12] and after[0].mapping[32 + 30:32 + 35].tolist() == [4, 5, 6, 11, 12]
    everything = np.zeros((1, 1, 8), np.uint32)
    everything[0, 0, 0] = 2
    everything[0, 0, 1:4] = np.asarray([260.0, 260.0, 1000.0], "f4").view(np.uint32)
    _, c = be.cut(dev(everything))
    assert c.cpu().numpy().tolist() == [[35, 35, 35, 0]] and be.summary().cpu().numpy()[0, 3] == 35.0
    be.reset()
    assert be.summary().cpu().numpy()[0, [1, 2, 3]].tolist() == [30.0, 5.0, 0.0], "reset: 30 slots, the five indices read removed, no flag"
    after2, res2, _ = check_against_ref(be, case, 0, what="sparse again")
    assert res2[0].tolist() == res[0].tolist() and be.summary().cpu().numpy()[0, [1, 2, 3]].tolist() == [35.0, 0.0, 0.0]
    assert_same(after2[0], after[0], "the same add after a reset: the same bits")
    be.frame()
    got = be.load_scene(0, after2[0].copy())
    assert got.beam_count == 35 and ref.alive_set(got)[[4, 5, 6, 11, 12]].all()
    assert_same(got, oracle_frames(oracle, after2[0], 1, OFF), "the frame after == oracle")
    be.destroy()


def test_lifecycle(sb):
    """7: reset, checkpoint, cut and fork around an add, through state_tensors, summary and bodies"""
    import torch
    case = cases.sparse_case(sb)
    rows, buf = case["rows"], case["bufs"][0]
    be = batch(sb, case)
    upload = raw(be)
    up_state, up_summary = upload[:3], np.frombuffer(upload[3], "f4").copy()
    # add -> reset: the upload's state bits; word 2 higher by the number added; the same add again gives the same result and bits
    r1, c1 = add(be, rows)
    first = raw(be)
    assert c1 == [[5, 0, 0, 0]] and first != upload
    be.reset()
    back = raw(be)
    s = np.frombuffer(back[3], "f4").copy()
    assert s[2] == up_summary[2] + 5 and np.array_equal(np.delete(s, 2).view("u4"), np.delete(up_summary, 2).view("u4"))
    p0, b0, a0 = (np.frombuffer(x, "u1") for x in up_state)
    p1, b1, a1 = (np.frombuffer(x, "u1") for x in back[:3])
    assert np.array_equal(p0, p1) and np.array_equal(a0, a1) and back[4:] == upload[4:], "particles, alive and bodies as uploaded"
    keep = np.ones(64, bool)
    keep[r1[0]] = False                        # (the five indices now export their inert rows: 'of the upload', not alive)
    assert np.array_equal(b0.reshape(64, 16)[keep], b1.reshape(64, 16)[keep])
    r2, c2 = add(be, rows)
    assert r2.tolist() == r1.tolist() and c2 == c1 and raw(be) == first
    # add -> checkpoint -> frames -> reset keeps the beams
    be.checkpoint()
    be.frame(2)
    be.reset()
    assert raw(be) == first and be.summary().cpu().numpy()[0, 1] == 35.0
    be.destroy()
    # cut -> frame -> add does not reuse the removed index; cut -> frame -> checkpoint -> add does
    for checkpoint, want in ((False, [4, 5, 6, 11, 12]), (True, [3, 4, 5, 6, 11])):
        be = batch(sb, case)
        one = np.zeros((1, 1, 8), np.uint32)   # a disc on the middle of beam slot 0 (data index 3): particles 0 and 1 of the rectangle
        one[0, 0, 0] = 2
        one[0, 0, 1:4] = np.asarray([200.0, 220.0, 1.0], "f4").view(np.uint32)
        hit, c = be.cut(dev(one), hit=True)
        assert c.cpu().numpy().tolist() == [[30, 1, 1, 0]] and hit.cpu().numpy()[0].nonzero()[0].tolist() == [3]
        be.frame()
        if checkpoint:
            be.checkpoint()
        now = load_all(be, case["bufs"])
        ra = [ref.alive_set(now[0] if checkpoint else buf)]
        _, res, cnt = check_against_ref(be, case, 0, before=now, reset_alive=ra, what="after a cut, checkpoint %s" % checkpoint)
        assert res[0].tolist() == want and be.summary().cpu().numpy()[0, [1, 2]].tolist() == [34.0, 0.0 if checkpoint else 1.0]
        be.destroy()
    # fork of a welded scene copies the weld; fork(as_reset=True) then reset keeps it
    two = dict(case, bufs=[buf, buf], rows=np.stack([rows[0], np.full_like(rows[0], -1)]))
    be = batch(sb, two)
    r, c = add(be, two["rows"])
    assert c == [[5, 0, 0, 0], [0, 0, 0, 0]] and r[1].tolist() == [ref.EMPTY] * 5
    welded = [x.cpu().numpy()[0].tobytes() for x in be.state_tensors()]
    be.fork(torch.tensor([0, 0], dtype=torch.int32, device="cuda"), as_reset=True)
    assert [x.cpu().numpy()[1].tobytes() for x in be.state_tensors()] == welded
    be.frame()
    be.reset(torch.tensor([0, 1], dtype=torch.uint8, device="cuda"))
    assert [x.cpu().numpy()[1].tobytes() for x in be.state_tensors()] == welded, "the forked state is the reset state"
    assert be.summary().cpu().numpy()[1, 1] == 35.0
    be.destroy()


def test_dry_run(sb):
    """8: result and counts are the real call's; no byte of the batch changes"""
    case = cases.default_case(sb)
    be = batch(sb, case)
    be.frame()
    before, scenes = raw(be), load_all(be, case["bufs"])
    dres, dcnt = add(be, case["rows"], SJ, dry=True)
    assert raw(be) == before
    for got, was in zip(load_all(be, case["bufs"]), scenes):
        assert_same(got, was, "a dry run")
    be.reset()                                  # (the reset blob too: a reset gives the upload)
    fresh = batch(sb, case)
    assert raw(be) == raw(fresh)
    for x in (be, fresh):
        x.frame()
    res, cnt = add(be, case["rows"], SJ)
    assert res.tolist() == dres.tolist() and cnt == dcnt and raw(be) != before
    be.destroy()
    fresh.destroy()


def test_contacts_compose_into_a_weld(sb, oracle):
    """9: contacts(pairs, other_body) -> new_beam_rows -> add_beams(length_current, skip_joined): two touching bodies become one"""
    case = cases.touching_case(sb)
    be = batch(sb, case, GRID)
    assert be.bodies()[1].cpu().numpy()[:, 0].tolist() == [2, 2]
    _, _, pairs = be.contacts(labels=True, pairs=8, other_body=True)
    assert pairs.cpu().numpy()[0].tolist() == [[2, 4], [3, 5]] + [[-1, -1]] * 6
    rows = sb.batch.new_beam_rows(pairs, *cases.MAT)
    assert rows.is_cuda and rows.cpu().numpy().tobytes() == ref.pack(
        [(a, b, 0.0) + cases.MAT for a, b in pairs.cpu().numpy().reshape(-1, 2)]).tobytes()
    res, cnt = be.add_beams(rows, length_current=True, skip_joined=True)
    assert res.cpu().numpy().tolist() == [[12, 13] + [ref.EMPTY] * 6] * 2 and cnt.cpu().numpy().tolist() == [[2, 0, 0, 0]] * 2
    assert be.bodies()[1].cpu().numpy()[:, 0].tolist() == [1, 1]
    res, cnt = be.add_beams(rows, length_current=True, skip_joined=True)
    assert res.cpu().numpy().tolist() == [[ref.JOINED] * 2 + [ref.EMPTY] * 6] * 2 and cnt.cpu().numpy().tolist() == [[0, 0, 2, 0]] * 2
    post = load_all(be, case["bufs"])
    be.step(1)
    r = oracle.OracleEngine(1000.0, 10.0, 64, 1, ALLPAIRS, threads=2)
    r.write_buffers(post[0])
    r.step(1)
    exp = r.load_buffers(post[0].copy())
    stress = be.state_tensors()[1].cpu().numpy()
    for s in range(2):
        assert stress[s, 12:14, 3].view("u4").tolist() == exp.beams["stress"][12:14].view("u4").tolist()
        assert stress[s, :14].view("u4").tolist() == np.stack([exp.beams[f][:14] for f in ("target_length", "last_length", "strain", "stress")], 1).view("u4").tolist()
    be.destroy()
