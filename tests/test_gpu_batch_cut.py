"""BatchEngine.cut (sb_batch_cut_device) on the GPU: twelve scenes of different sizes -- one at full capacity, one
never uploaded, two with only CUT_NONE shapes -- each cut by its own shapes in one launch.  `hit` and `counts` equal tests/cut_ref.py
and Engine.cut per scene; untouched scenes stay bit-identical; cut + frame equals the oracle with the hit slots' delete bits set, with
the contact cells and with the walk; reset undoes a cut, fork copies a pending one, checkpoint keeps it, a rollout after it equals
the individual calls."""
import numpy as np
import pytest

import cut_cases
import cut_ref
from batch_harness import load_all, upload_each
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

OFF, ALLPAIRS, GRID = 0, 1, 2
MODES = [pytest.param(GRID, id="grid"), pytest.param(ALLPAIRS, id="walk")]


@pytest.fixture(scope="module")
def scenes(sb):
    return cut_cases.batch_scenes(sb)


def batch(sb, bufs, mode=GRID):
    be = sb.BatchEngine(n_scenes=len(bufs), layout=2, max_particles=cut_cases.BATCH_CAP[0], max_beams=cut_cases.BATCH_CAP[1], collision_mode=mode)
    upload_each(be, bufs)
    return be


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def refs(bufs, shapes, dry=False):
    """per scene (hit, counts) of the reference on buffers as read back; a scene never uploaded: nothing"""
    out = []
    for b, sh in zip(bufs, shapes):
        out.append((np.zeros(cut_cases.BATCH_CAP[1], np.uint8), [0, 0, 0, 0]) if b is None else cut_ref.scene_ref(b, sh, dry=dry))
    return out


def raw_state(be):
    p, b, a = be.state_tensors()
    return [x.cpu().numpy().tobytes() for x in (p, b, a)]


def assert_all_same(got, exp, what):
    for i, (g, e) in enumerate(zip(got, exp)):
        if e is not None:
            assert_same(g, e, "%s: scene %d" % (what, i))


def oracles(oracle, bufs, mode):
    out = []
    for b in bufs:
        if b is None:
            out.append(None)
            continue
        r = oracle.OracleEngine(1000.0, 10.0, 64, 2, mode, threads=4)
        r.write_buffers(b)
        out.append(r)
    return out


def flag(ref, buf, shapes):
    now = ref.load_buffers(buf.copy())
    _, A, B = cut_ref.beam_ends(now)
    for s in np.flatnonzero(cut_ref.hits(shapes, A, B)):
        bit = buf.max_particles + int(s)
        ref.delete[bit >> 5] |= np.uint32(1 << (bit & 31))


@pytest.mark.parametrize("mode", MODES)
def test_hit_counts_and_the_frames_after(sb, oracle, scenes, mode):
    import torch
    bufs, shapes = scenes
    be, plain = batch(sb, bufs, mode), batch(sb, bufs, mode)
    # (ALLPAIRS for both modes on purpose: the batch's cells and its walk both give the bits of the reference's all-pairs loop,
    # tests/test_gpu_batch_grid.py; the oracle's own grid mode is another implementation of the same bits and is not needed here)
    rs = oracles(oracle, bufs, ALLPAIRS)
    for x in [be, plain] + [r for r in rs if r is not None]:
        x.step(5)
    now = load_all(be, bufs)
    before = raw_state(be)
    # a dry run first: reports, changes nothing
    want = refs(now, shapes, dry=True)
    hit = torch.full((len(bufs), be.max_beams), 0xA5, dtype=torch.uint8, device="cuda")
    _, counts = be.cut(dev(shapes), dry_run=True, hit=hit)
    assert np.array_equal(hit.cpu().numpy(), np.stack([w[0] for w in want])), "hit (zero-filled over max_beams for every scene)"
    assert counts.cpu().numpy().tolist() == [w[1] for w in want]
    assert raw_state(be) == before
    # for real
    want = refs(now, shapes)
    hit, counts = be.cut(dev(shapes), hit=True)
    assert np.array_equal(hit.cpu().numpy(), np.stack([w[0] for w in want]))
    assert counts.cpu().numpy().tolist() == [w[1] for w in want]
    assert sum(w[1][1] > 0 for w in want) >= 7 and want[3][1] == [0, 0, 0, 0] and want[6][1][1] == 0 and want[9][1][1] == 0
    assert raw_state(be) == before, "a cut writes flags only"
    pending = be.summary().cpu().numpy()[:, 3]
    assert pending.tolist() == [float(w[1][1]) for w in want], "summary: pending flags per scene"
    # Engine.cut on the same scene
    for i in (1, 2, 5):
        eng = sb.Engine(layout=2, max_particles=be.max_particles, max_beams=be.max_beams, collision_mode=OFF)
        eng.write_buffers(now[i])
        h, c = eng.cut(dev(shapes[i]), hit=True)
        assert np.array_equal(h.cpu().numpy(), want[i][0]) and c.cpu().numpy().tolist() == want[i][1], i
        eng.destroy()
    # the frames after: the oracle with the bits set; scenes the cut left alone equal the batch that was never cut
    for r, b, sh in zip(rs, bufs, shapes):
        if r is not None:
            flag(r, b, sh)
    for x in (be, plain):
        x.step(x.subticks - 5)
        x.delete_pass()
        x.frame()
    for r in rs:
        if r is not None:
            r.step(r.subticks - 5)
            r.delete_pass()
            r.frame()
    got, unc = load_all(be, bufs), load_all(plain, bufs)
    assert_all_same(got, [None if r is None else r.load_buffers(b.copy()) for r, b in zip(rs, bufs)], "cut + frames == oracle")
    for i in (6, 9):
        assert_same(got[i], unc[i], "scene %d (only CUT_NONE) == never cut" % i)
    for a, b in zip(be.state_tensors(), plain.state_tensors()):   # the state rows of the scenes left alone, never uploaded included
        assert torch.equal(a[[3, 6, 9]].view(torch.uint8), b[[3, 6, 9]].view(torch.uint8))
    assert got[2].beam_count <= cut_cases.BATCH_CAP[1] - want[2][1][1] < unc[2].beam_count
    if mode == GRID:
        assert be.info("cell_substeps") > 0
    be.destroy()
    plain.destroy()


def test_reset_fork_checkpoint_rollout(sb, scenes):
    import torch
    bufs, shapes = scenes
    n = len(bufs)
    sh = dev(shapes)
    be, plain = batch(sb, bufs), batch(sb, bufs)
    # reset undoes a cut
    be.cut(sh)
    be.reset()
    for x in (be, plain):
        x.frame()
    assert_all_same(load_all(be, bufs), load_all(plain, bufs), "reset undoes a cut")
    # checkpoint after a cut makes it the reset state; a rollout after a cut equals the individual calls
    _, c1 = be.cut(sh)
    be.checkpoint()
    be.frame(2)
    two = load_all(be, bufs)
    be.reset()
    assert be.summary().cpu().numpy()[:, 3].tolist() == c1.cpu().numpy()[:, 1].astype(float).tolist(), "the pending cut is the reset state"
    rows = be.rollout(frames=2)
    assert_all_same(load_all(be, bufs), two, "rollout after a cut == frames after a cut")
    assert rows.shape == (2, n, 24)
    plain.cut(sh)
    plain.frame(2)
    assert_all_same(load_all(plain, bufs), two, "checkpoint keeps a pending cut")
    # fork copies a pending cut: scene 0 <- scene 7 with its flags pending; both then lose the same beams
    be.reset()                                     # (back to the cut, pending)
    src = torch.arange(n, dtype=torch.int32, device="cuda")
    src[0] = 7
    be.fork(src)
    _, c = be.cut(sh[:, :0], hit=False)            # k = 0: counts only
    assert c.cpu().numpy()[:, 1:].tolist() == [[0, 0, 0]] * n
    assert be.summary().cpu().numpy()[[0, 7], 3].tolist() == [float(c1[7, 1])] * 2 and int(c1[7, 1]) > 0
    again = be.cut(sh, dry_run=True)[1].cpu().numpy()
    assert again[7].tolist() == [int(c1[7, 0]), int(c1[7, 1]), 0, int(c1[7, 1])], "already flagged"
    be.frame()
    got = load_all(be, bufs)
    assert_same(got[0], got[7], "the fork of a scene with a pending cut")
    assert got[7].beam_count <= bufs[7].beam_count - int(c1[7, 1])
    be.destroy()
    plain.destroy()


def test_errors(sb, scenes):
    import ctypes
    import torch
    from softbody_webgpu_amd.engine import EngineError
    bufs, shapes = scenes
    be = batch(sb, bufs[:2])
    lib = sb.batch.load_library()
    vp = ctypes.c_void_p
    sh = dev(np.zeros((2, 65, 8), np.uint32))
    counts = torch.zeros(9, dtype=torch.int32, device="cuda")
    for flags, ptr, k, cptr in ((2, sh.data_ptr(), 1, None), (0, sh.data_ptr(), 65, None), (0, None, 1, None), (0, sh.data_ptr() + 1, 1, None),
                                (0, sh.data_ptr(), 1, counts.data_ptr() + 2)):
        assert lib.sb_batch_cut_device(be._h, flags, vp(ptr), k, None, vp(cptr)) == 1
    with pytest.raises(ValueError):
        be.cut(sh)                                  # k = 65
    with pytest.raises(ValueError):
        be.cut(sh[:1, :3])                          # one scene's shapes for two scenes
    assert be.info("cut_kernel_vgprs") > 0
    _, c = be.cut(dev(shapes[:2]), hit=False)
    assert c.cpu().numpy()[:, 1].min() > 0
    be.destroy()
