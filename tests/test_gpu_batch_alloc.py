"""The free-index allocator of the batch's adding calls (csrc/sb_batch_alloc.h) from both kernels in one process, on the GPU, at the
smallest capacities whose bitmaps have a partial last word and a second and third word: add_particles and then add_beams onto the
spawned particles, in scenes whose free data indices are only the last one, none, all but index 0, and in a scene never uploaded.
result, counts and the scene read back are compared bit for bit with tests/batch_add_particles_ref.py and
tests/batch_add_beams_ref.py chained; then reset(), and the same two calls once more."""
import numpy as np
import pytest

import batch_add_beams_cases as beam_cases
import batch_add_beams_ref as beam_ref
import batch_add_particles_ref as ref
from batch_harness import load_all, make_batch, upload_each
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

CAPS = [(37, 61), (33, 65)]
K = 8
KINDS = ("last", "none", "all-but-0", "never")


def scene(sb, cap, kind, rng):
    """a scene whose free particle AND beam data indices are what `kind` says; rng: shuffles the slot order (None: ascending).
    Beam slot s joins the s-th pair of particle slots; "all-but-0" has one particle, so its one beam joins that particle to itself
    (an upload takes it, and nothing here steps the scene)."""
    maxP, maxB = cap
    if kind == "never":
        return None
    pd = {"last": np.arange(maxP - 1), "none": np.arange(maxP), "all-but-0": np.arange(1)}[kind]
    bd = {"last": np.arange(maxB - 1), "none": np.arange(maxB), "all-but-0": np.arange(1)}[kind]
    if rng is not None:
        pd, bd = rng.permutation(pd), rng.permutation(bd)
    P = len(pd)
    pairs = [(i, j) for i in range(P) for j in range(i + 1, P)] if P > 1 else [(0, 0)]
    _, template = sb.scenes.rectangle(200.0, 200.0, 40.0, 2, 2, 50.0, 700.0, 0.2, 1.0e9, layout=2)
    buf = sb.Buffers(2, maxP, maxB)
    s = np.arange(P)
    buf.particles[pd, 0], buf.particles[pd, 1] = 40.0 + 40.0 * (s % 8), 40.0 + 40.0 * (s // 8)
    for slot, d in enumerate(bd):
        rec = template[0].copy()
        a, b = pairs[slot]
        rec["a"], rec["b"] = pd[a], pd[b]
        buf.beams[d] = rec
    buf.mapping[:P] = pd
    buf.mapping[maxP:maxP + len(bd)] = bd
    buf.particle_count, buf.beam_count = P, len(bd)
    return buf


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def weld_rows(bufs, res):
    """K rows per scene that name the spawned indices: row j joins result[j] -- where that row found no room, the particle of slot
    j -- to the particle of slot j + 1 (mod P)"""
    out = []
    for i, b in enumerate(bufs):
        if b is None:
            out.append(beam_ref.pack([(j, j + 1, 30.0) + beam_cases.MAT for j in range(K)]))
            continue
        pd = b.mapping[:b.particle_count].astype(np.int64)
        out.append(beam_ref.pack([(int(res[i][j]) if res[i][j] >= 0 else int(pd[j % len(pd)]), int(pd[(j + 1) % len(pd)]), 30.0) + beam_cases.MAT
                                  for j in range(K)]))
    return np.stack(out)


@pytest.mark.parametrize("cap", CAPS, ids=lambda c: "%dx%d" % c)
def test_spawn_then_weld_at_the_edge_words(sb, cap):
    maxP, maxB = cap
    rng = np.random.default_rng(maxP)
    bufs = [scene(sb, cap, kind, None) for kind in KINDS] + [scene(sb, cap, kind, rng) for kind in KINDS]
    case = dict(layout=2, cap=cap, bufs=bufs, mode=0)
    be = make_batch(sb, case, mode=0)
    upload_each(be, bufs)
    prow = np.stack([ref.pack([(i, 100.0 + 50.0 * j, 800.0 + 10.0 * i, 0.5, -0.5) for j in range(K)]) for i in range(len(bufs))])
    reset_alive = [None if b is None else beam_ref.alive_set(b) for b in bufs]
    FULL, INV = ref.FULL, ref.INVALID
    first = None
    for episode in range(2):
        # (the scenes as read back: after a reset the record of an undone weld keeps its material, which no rule looks at)
        before = load_all(be, bufs)
        # ---- spawn
        res, cnt = (x.cpu().numpy() for x in be.add_particles(dev(prow)))
        want = [ref.add_ref(b, prow[i]) for i, b in enumerate(before)]
        for i, (_, r, c) in enumerate(want):
            print("episode", episode, "spawn scene", i, res[i].tolist(), r.tolist(), cnt[i].tolist(), c)
        for i, (_, r, c) in enumerate(want):
            assert res[i].tolist() == r.tolist() and cnt[i].tolist() == c, (episode, i)
        spawned = load_all(be, bufs)
        for i, (edited, _, _) in enumerate(want):
            if edited is not None:
                assert_same(spawned[i], edited, "episode %d scene %d after the spawn == the restatement's edit" % (episode, i))
        # ---- weld onto the spawned particles
        brow = weld_rows(bufs, res)
        bres, bcnt = (x.cpu().numpy() for x in be.add_beams(dev(brow)))
        bwant = [beam_ref.add_ref(b, brow[i], 0, reset_alive[i]) for i, b in enumerate(spawned)]
        for i, (_, r, c) in enumerate(bwant):
            print("episode", episode, "weld scene", i, bres[i].tolist(), r.tolist(), bcnt[i].tolist(), c)
        for i, (_, r, c) in enumerate(bwant):
            assert bres[i].tolist() == r.tolist() and bcnt[i].tolist() == c, (episode, i)
        welded = load_all(be, bufs)
        for i, (edited, _, _) in enumerate(bwant):
            if edited is not None:
                assert_same(welded[i], edited, "episode %d scene %d after the weld == the restatement's edit" % (episode, i))
        # ---- what the scenes are built for
        for i in (0, 4):
            assert res[i].tolist() == [maxP - 1] + [FULL] * 7 and bres[i].tolist() == [maxB - 1] + [FULL] * 7, "only the last index"
        for i in (1, 5):
            assert res[i].tolist() == [FULL] * K == bres[i].tolist(), "no index"
        for i in (2, 6):
            assert res[i].tolist() == list(range(1, 9)) == bres[i].tolist(), "index 0 is taken"
        for i in (3, 7):
            assert res[i].tolist() == [INV] * K == bres[i].tolist(), "never uploaded"
        if first is None:
            first = (res.tobytes(), cnt.tobytes(), bres.tobytes(), bcnt.tobytes())
        else:
            assert first == (res.tobytes(), cnt.tobytes(), bres.tobytes(), bcnt.tobytes()), "the reset gave every index back"
        # ---- reset: the spawned particles and the welds onto them are gone
        be.reset()
        back = load_all(be, bufs)
        for i, b in enumerate(before):
            if b is None:
                continue
            want_back, _ = ref.reset_ref(welded[i], b, b.particle_count)
            got = back[i]
            assert got.metadata.tobytes() == want_back.metadata.tobytes() and got.mapping.tobytes() == want_back.mapping.tobytes(), (episode, i)
            assert got.particles.tobytes() == want_back.particles.tobytes(), (episode, i)
            alive = np.flatnonzero(reset_alive[i])
            assert got.beams[alive].tobytes() == b.beams[alive].tobytes() and got.beam_count == b.beam_count, (episode, i)
    be.destroy()
