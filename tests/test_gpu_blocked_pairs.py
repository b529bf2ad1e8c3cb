"""The blocked kernel's entry slots pair up NEIGHBOURS of a tile's entry list (csrc/sb_blocked.hip SB_ENT_L: a group of two
slots runs when its first entry is inside the substep's prefix), so the slot <-> list-index mapping is no longer `tid + i T`.
Bit for bit against the oracle -- particles, beam target / last length, strain / stress of the last substep of a call, the
counts -- at the smallest shapes where that mapping can go wrong: odd and even own-beam counts (a pair straddling the tile's
own beams), tiles whose ranges of the plan arrays start at odd offsets, halo prefixes that end inside a pair for every launch
depth up to K (material modes 2 and 1, and the tracked variant under the spatial hash), and yield / break / delete."""
import numpy as np
import pytest

from test_gpu_parity import GRID, OFF, TILED, assert_same

pytestmark = pytest.mark.gpu


def engines(sb, oracle, buf, *, K=0, tile=0, bounds=4000.0, mode=OFF):
    eng = sb.Engine(bounds_size=bounds, subticks=64, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams,
                    collision_mode=mode, path=TILED if mode == OFF else 0, tile_particles=tile, block_substeps=K)
    ref = oracle.OracleEngine(bounds, 10.0, 64, buf.layout, mode, threads=8)
    eng.write_buffers(buf)
    ref.write_buffers(buf)
    return eng, ref


def step_and_compare(eng, ref, buf, calls, what):
    """Every call ends with the strain / stress variant of the kernel; compared after each."""
    for n in calls:
        eng.step(n)
        ref.step(n)
        assert_same(eng.load_buffers(buf.copy()), ref.load_buffers(buf.copy()), "%s, after step(%d)" % (what, n))


@pytest.mark.parametrize("w,h,odd", [(5, 5, False), (6, 5, True)])
def test_one_tile_with_an_even_and_an_odd_own_beam_count(sb, oracle, w, h, odd):
    buf = sb.scenes.lattice_buffers(w, h, d=25.0, origin=(100.0, 100.0), jitter=2.0, layout=2, strain_limit=1e9, velocity=(1.0, -2.0))
    assert (buf.beam_count % 2 == 1) == odd
    eng, ref = engines(sb, oracle, buf, K=3, tile=1024)
    assert eng.info("tiles") == 1 and eng.info("substeps_per_launch") == 3
    step_and_compare(eng, ref, buf, (1, 7, 3), "%d x %d, one tile" % (w, h))
    eng.destroy()


def two_blobs(sb, first, second, gap=200.0):
    (w0, h0), (w1, h1) = first, second
    a = sb.scenes.lattice_buffers(w0, h0, d=25.0, origin=(100.0, 100.0), jitter=2.0, layout=2, strain_limit=1e9, velocity=(1.0, -2.0))
    b = sb.scenes.lattice_buffers(w1, h1, d=25.0, origin=(100.0 + 25.0 * w0 + gap, 100.0), jitter=2.0, layout=2, strain_limit=1e9,
                                  velocity=(-1.0, -2.0), seed=7)
    Pa, Ba, Pb, Bb = a.particle_count, a.beam_count, b.particle_count, b.beam_count
    beams = np.concatenate([a.beams[:Ba], b.beams[:Bb]])
    beams["a"][Ba:] += Pa
    beams["b"][Ba:] += Pa
    buf = sb.Buffers(2, Pa + Pb, Ba + Bb)
    buf.set_scene(np.concatenate([a.particles[:Pa], b.particles[:Pb]]), beams)
    return buf


def test_tiles_whose_plan_ranges_start_at_odd_offsets(sb, oracle):
    """A 6 x 5 blob (69 beams) in front of a 40 x 40 one that splits into several tiles: the later tiles' first own beam, first
    entry and first halo state index are odd for some of them (plan_odd_offsets: bits 0, 1, 2)."""
    buf = two_blobs(sb, (6, 5), (40, 40))
    eng, ref = engines(sb, oracle, buf, K=4, tile=300)
    odd = eng.info("plan_odd_offsets")
    if odd != 7:
        eng.destroy()
        pytest.skip("no tile with odd b0, e0 and s0 in this plan (plan_odd_offsets = %d)" % odd)
    assert eng.info("tiles") >= 3 and eng.info("substeps_per_launch") == 4
    step_and_compare(eng, ref, buf, (1, 9, 4), "odd offsets")
    eng.destroy()


CALLS = (1, 7, 13, 20)   # with a depth the caller names a call runs in the fewest launches: every depth up to K occurs


def lattice70(sb, rest_current=False):
    buf = sb.scenes.lattice_buffers(70, 70, d=30.0, origin=(300.0, 900.0), jitter=1.0, layout=2, velocity=(0.4, -1.0))
    return sb.scenes.rest_at_current_length(buf) if rest_current else buf


@pytest.mark.parametrize("K", [2, 3, 6, 7])
@pytest.mark.parametrize("mat", [2, 1])
def test_halo_prefix_ends_inside_a_pair(sb, oracle, K, mat):
    """70 x 70 with the engine's own tile size (some twenty tiles, rings all around): the halo prefix of a substep ends
    wherever the rings put it -- inside a pair, at a wave's boundary, at a group's."""
    buf = lattice70(sb, rest_current=mat == 1)
    eng, ref = engines(sb, oracle, buf, K=K)
    assert eng.info("material_mode") == mat and eng.info("tiles") >= 4 and eng.info("plan_depth") == K
    step_and_compare(eng, ref, buf, CALLS, "70 x 70, K = %d, material mode %d" % (K, mat))
    eng.destroy()


def test_tracked_variant_on_the_quiet_scene(sb, oracle):
    """The same lattice under the spatial hash: nothing is within reach of anything, so after the stretch of single substeps
    that builds the hash the calls run as tracked blocked launches."""
    buf = lattice70(sb)
    eng, ref = engines(sb, oracle, buf, mode=GRID, bounds=6000.0)
    step_and_compare(eng, ref, buf, CALLS + (100,), "70 x 70, spatial hash")
    assert eng.info("hybrid_substeps") > 0
    eng.destroy()


@pytest.mark.parametrize("tile", [1024, 64])
def test_yield_break_and_delete_with_an_odd_own_beam_count(sb, oracle, tile):
    """A 15 x 12 lattice (487 beams) thrown into the corner: beams yield, cross their break limit and are removed by the
    delete pass of a frame -- in one tile that owns all 487, and cut into small tiles that hold copies of each other's dead
    beams; then more substeps on what is left."""
    buf = sb.scenes.lattice_buffers(15, 12, d=30.0, origin=(30.0, 30.0), spring=50.0, damp=100.0, yield_strain=0.05, strain_limit=0.12,
                                    layout=1, velocity=(-40.0, -35.0), slack=8)
    assert buf.beam_count % 2 == 1
    eng, ref = engines(sb, oracle, buf, K=3, tile=tile, bounds=1000.0)
    assert (eng.info("tiles") == 1) == (tile == 1024)
    step_and_compare(eng, ref, buf, (5,), "before the first delete pass")
    for _ in range(3):
        eng.frame()
        ref.frame()
    exp = ref.load_buffers(buf.copy())
    assert exp.beam_count < buf.beam_count, "scene must break beams"
    assert (exp.beams["target_length"][:exp.beam_count] != exp.beams["length"][:exp.beam_count]).any(), "scene must yield"
    assert_same(eng.load_buffers(buf.copy()), exp, "after three frames")
    step_and_compare(eng, ref, buf, (5, 2), "after the delete passes")
    eng.destroy()
