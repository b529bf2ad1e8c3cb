"""Engine.raycast (sb_raycast_device) at its widths: n_rays of 0, 1, 63, 64, 65, 257 and 4097 on one lattice; data
indices past 2^16 -- about 6000 particles at capacity 2^18 + 4096 with data indices drawn as contacts_cases.indices_past_2_18 draws
them, their beams at data indices from 65 536 on: a key with 16 bits of index cannot name the winners.  Bit for bit against
tests/raycast_ref.py."""
import numpy as np
import pytest

import batch_raycast_ref as bref
import contacts_cases as cc
import graph_cases
import raycast_ref as ref
import report_harness as rh
from test_gpu_raycast import BOUNDS, cast, check, lattice, lattice_rows

pytestmark = pytest.mark.gpu

OFF = 0


@pytest.fixture(scope="module")
def lattice_engine(sb):
    buf = lattice(sb, 24, 24)
    eng = rh.engine(sb, buf, BOUNDS, collision_mode=OFF)
    rows = np.concatenate([lattice_rows(buf, 21 + k, 512) for k in range(8)])[:4097]
    now = eng.load_buffers(buf.copy())
    want = ref.raycast_ref(now, rows, BOUNDS, 10.0)
    yield eng, rows, want
    eng.destroy()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_widths(lattice_engine, n):
    eng, rows, want = lattice_engine
    if n == 0:
        z = eng.raycast_host(rows[:0])
        assert z.t.shape == (0,) and not z.counts.any()
        return
    got = cast(eng, rows[:n])
    exp = ref.RayCast(want.t[:n], want.hit[:n], None)
    assert ref.same(ref.RayCast(got.t, got.hit, None), exp) == [], n
    kinds = want.hit[:n, 0]
    assert got.counts[:4].tolist() == [(kinds >= 0).sum(), (kinds == 1).sum(), (kinds == 2).sum(), (kinds == 3).sum()]
    assert got.counts[4] == sum(1 for w in rows[:n] if bref.verdict(w, False) == 0 and not ref.walkable(w, BOUNDS)) and got.counts[5:].tolist() == [0, 0, 0]


def test_indices_past_2_16(sb):
    cap = cc.SECOND_TRIP + 4096
    among = np.concatenate([np.arange(0, cc.SECOND_TRIP, 64), np.arange(cc.SECOND_TRIP, cap)])
    rng = np.random.default_rng(67)
    n, per_row = 6000, 80
    pmap = among[rng.permutation(len(among))[:n]]
    k = np.arange(n)
    pairs = np.stack([k[k % per_row != per_row - 1], k[k % per_row != per_row - 1] + 1], 1)
    max_beams = 65536 + 8192
    bmap = 65536 + rng.permutation(8192)[:len(pairs)]
    buf = graph_cases.scene(sb, (cap, max_beams), n, pairs, layout=2, pmap=pmap, bmap=bmap, lengths=30.0)
    buf.particles[pmap, :2] = cc.jittered_grid(n, per_row, (40.0, 40.0), seed=66, spacing=30.0, jitter=2.0)
    bounds = 2600.0
    eng = rh.engine(sb, buf, bounds, collision_mode=OFF)
    rows = []
    for j in range(192):
        o = rng.uniform(30.0, 2300.0, 2)
        rows.append(((1, 2, 7)[j % 3], o[0], o[1], *rng.normal(size=2), ref.INF))
    rows = bref.pack(rows)
    _, got = check(eng, buf, rows, None, "indices past 2^16", bounds=bounds)
    part, beam = got.hit[got.hit[:, 0] == 1, 1], got.hit[got.hit[:, 0] == 2, 1]
    assert part.size > 20 and beam.size > 20 and (part >= 65536).any() and (beam >= 65536).all(), "a 16-bit index cannot name these winners"
    lab = eng.bodies()[0].cpu().numpy()
    _, got = check(eng, buf, rows, lab, "indices past 2^16, labelled", bounds=bounds)
    assert (got.hit[got.hit[:, 0] == 2, 2] >= 0).all()
    eng.destroy()
