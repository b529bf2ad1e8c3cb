"""Engine.nearest (sb_nearest_device) at its widths: n = 1, 63, 64, 65, 255, 257 and 1000 rows on one 16 x 16 lattice,
with more swept rows than a tile of the sweep holds (64) from 255 rows on; every word of every output is written over a pattern.  Bit
for bit against tests/nearest_ref.py."""
import numpy as np
import pytest

import nearest_ref as ref
import report_harness as rh
from test_gpu_nearest import ask, lattice_points
from test_gpu_raycast import BOUNDS, lattice

pytestmark = pytest.mark.gpu

OFF = 0
PATTERN = {"d": np.float32(-7.25).view(np.uint32), "hit": np.int32(-1515870811).view(np.uint32), "point": np.float32(-3.5).view(np.uint32),
           "within": np.int32(-99).view(np.uint32)}


@pytest.fixture(scope="module")
def lattice_engine(sb):
    buf = lattice(sb, 16, 16)
    eng = rh.engine(sb, buf, BOUNDS, collision_mode=OFF)
    rows = np.concatenate([lattice_points(21 + k, 160) for k in range(7)])[:1000]
    rows[::3, 3] = np.float32(ref.INF).view(np.uint32)   # a third of the rows reach everything: with within the sweep answers them
    now = eng.load_buffers(buf.copy())
    swept = []
    want = ref.nearest_ref(now, rows, BOUNDS, 10.0, swept=swept)
    yield eng, rows, want, swept
    eng.destroy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1000])
def test_widths(lattice_engine, n):
    eng, rows, want, swept = lattice_engine
    got = ask(eng, rows[:n])
    exp = ref.Nearest(want.d[:n], want.hit[:n], want.point[:n], want.within[:n], None)
    assert ref.same(got, exp, skip=("counts",)) == [], n
    valid = want.hit[:n, 0] >= 0
    for name in ("d", "hit", "point", "within"):   # a valid row never answers the pattern's bits: every word was written
        assert not (getattr(got, name).view(np.uint32).reshape(n, -1)[valid] == PATTERN[name]).any(), name
    kinds = want.hit[:n, 0]
    assert got.counts[:4].tolist() == [(kinds >= 0).sum(), (kinds == 1).sum(), (kinds == 2).sum(), (kinds == 3).sum()]
    assert got.counts[4] == sum(swept[:n]) and (n < 255 or got.counts[4] > 65), "more swept rows than one tile of the sweep from 255 rows on"
    assert got.counts[5:].tolist() == [0, 0, 0]
