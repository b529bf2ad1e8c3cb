"""BatchEngine.raycast across its widths, bit for bit against tests/batch_raycast_ref.py: every split of the
workgroup into parts (k = 1, 63, 64, 65, 255, 256: 256, 4, 4, 2, 1 and 1 parts, with and without padding lanes), the capacity
corner (1024 particles / 4096 beams, the last slot of each list met), odd capacities, an uploaded scene of no particles, and a batch
of more workgroups than the device holds at once."""
import numpy as np
import pytest

import batch_add_beams_cases as add_cases
import batch_raycast_cases as cases
import batch_raycast_ref as ref
from batch_harness import make_batch
from batch_query_rig import batch
from test_gpu_batch_raycast import check

pytestmark = pytest.mark.gpu

INF = ref.INF


def drawn(buf, k, seed, **kw):
    """k packed rows of cases.drawn_rows over `buf` with bodies()'s labels of it"""
    rng = np.random.default_rng(seed)
    lab = ref.bodies_labels(buf)
    rows = []
    while len(rows) < k:
        rows += cases.drawn_rows(buf, rng, lab, **kw)
    return ref.pack(rows[:k])


@pytest.mark.parametrize("k", [1, 63, 64, 65, 255, 256])
def test_every_part_split(sb, k):
    """1: the default scene, the full-capacity lattice of the case set and a never-uploaded scene under k rays, with labels"""
    cs = cases.case_set(sb)
    bufs = [cs[4]["buf"], cs[11]["buf"], None]
    rows = np.stack([drawn(bufs[0], k, 100 + k), drawn(bufs[1], k, 200 + k), drawn(bufs[0], k, 300 + k, outside=True)])
    labels = np.stack([cs[4]["labels"], cs[11]["labels"], cs[9]["labels"]])
    be = batch(sb, bufs)
    _, got = check(be, bufs, rows, labels, "k = %d" % k)
    if k >= 63:
        assert (got.counts[:2, 1:] > 0).all() and got.counts[2, 1:3].tolist() == [0, 0] and got.counts[2, 3] > 0
    check(be, bufs, rows, None, "k = %d, no labels" % k)
    be.destroy()


def test_capacity_corner(sb):
    """2: 1024 particles / 4096 beams under shuffled mappings and 256 rays; rows 0 and 1 meet the particle and the beam in the LAST
    slot of their lists"""
    buf = add_cases.big_scene(sb, 4096, 32)
    maxP, maxB = add_cases.BIG_CAP
    assert (buf.particle_count, buf.beam_count) == (maxP, maxB)
    last_p, last_b = int(buf.mapping[maxP - 1]), int(buf.mapping[maxP + maxB - 1])
    x, y = (float(v) for v in buf.particles[last_p, :2])
    pa, pb = (buf.particles[int(buf.beams[e][last_b]), :2].astype(np.float64) for e in ("a", "b"))
    q = 0.75 * pa + 0.25 * pb     # a quarter along: no other beam of the lattice passes there
    e = (pb - pa) / np.hypot(*(pb - pa))
    n = np.array([-e[1], e[0]])
    special = ref.pack([(ref.PARTICLES, x + 12.0, y + 3.0, -1, 0, 30.0), (ref.BEAMS, *(q + 2.0 * n), *(-n), 4.0)])
    rows = np.concatenate([special, drawn(buf, 254, 7)])[None]
    labels = ref.bodies_labels(buf)[None]
    be = batch(sb, [buf], cap=add_cases.BIG_CAP)
    _, got = check(be, [buf], rows, labels, "capacity corner")
    assert got.hit[0, 0, :2].tolist() == [1, last_p] and got.hit[0, 1, :2].tolist() == [2, last_b], (got.hit[0, :2], last_p, last_b)
    assert (got.counts[0, 1:] > 10).all()
    check(be, [buf], rows, None, "capacity corner, no labels")
    be.destroy()


@pytest.mark.parametrize("cap", add_cases.ODD_CAPS)
def test_odd_capacities(sb, cap):
    """3: capacities 33 / 37 and 65 / 61, the last particle at data index max_particles - 1; beside it an uploaded scene of no
    particles and no beams, and a never-uploaded one: walls only"""
    buf = add_cases.odd_case(sb, cap)["bufs"][0]
    empty = sb.Buffers(cases.LAYOUT, *cap)
    bufs = [buf, empty, None]
    x, y = (float(v) for v in buf.particles[cap[0] - 1, :2])
    rows = np.stack([np.concatenate([ref.pack([(ref.PARTICLES, x, y - 25.0, 0, 1, INF)]), drawn(buf, 36, cap[0], outside=bool(i))]) for i in range(3)])
    labels = np.stack([ref.bodies_labels(buf), np.full(cap[0], -1, np.int32), np.full(cap[0], -1, np.int32)])
    be = batch(sb, bufs, cap=cap)
    _, got = check(be, bufs, rows, labels, "odd capacity %s" % (cap,))
    assert got.hit[0, 0].tolist() == [1, cap[0] - 1, int(labels[0, cap[0] - 1])] and got.t[0, 0] == 15.0
    assert (got.counts[1:, 1:3] == 0).all() and (got.counts[1:, 3] > 0).all()
    be.destroy()


def test_more_workgroups_than_fit(sb):
    """4: 300 default scenes, each with its own eight rays"""
    buf = cases.case_set(sb)[4]["buf"]
    n = 300
    pool = drawn(buf, 64, 11)
    rows = np.stack([np.roll(pool, -i, axis=0)[:8] for i in range(n)])
    be = make_batch(sb, dict(layout=cases.LAYOUT, cap=cases.CAP, bufs=[buf], mode=0), n=n, mode=0)
    be.write_scene(buf)
    check(be, [buf] * n, rows, np.stack([ref.bodies_labels(buf)] * n), "300 scenes")
    be.destroy()
