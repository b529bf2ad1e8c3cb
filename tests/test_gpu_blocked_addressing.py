"""The blocked kernel's load and store phases behind their accessors (csrc/sb_blocked.hip SbMem; flat addresses, or range-checked
buffer instructions in a library built with SB_BK_BUFFER=1 -- sb_get_info blocked_addressing says which, 0 or 1, and the tests hold
for either): the blocked engine against the same engine with block_substeps=1 (the single-substep kernels), bit for bit
-- particles, target / last length, strain, stress, the counts (a beam whose break bit is raised is gone after the frame's delete
pass) -- after step(k) for every k in 1 .. 7 and after one call of 20 (7 + 7 + 6: lean launches, then the strain / stress variant),
at the smallest shapes at which each offset can go wrong: partial waves and an almost empty halo slot, one tile with no halo at
all (every halo request out of range), dead entries beside live ones, a yielded tile beside pristine ones, live accelerations,
material mode 1 (ent_length), the wide word, and arrays that end exactly at the last tile's last element."""
import numpy as np
import pytest

from test_gpu_parity import OFF, TILED, assert_same

pytestmark = pytest.mark.gpu
FLAT, BUFFER = 0, 1
CALLS = (1, 2, 3, 4, 5, 6, 7, 20)


def lattice(sb, **kw):
    """37 x 29: 1073 particles -- with 256-particle tiles n_own is no multiple of 64 and a halo is shorter than one slot of 512."""
    kw.setdefault("origin", (300.0, 900.0))
    kw.setdefault("velocity", (0.4, -1.0))
    return sb.scenes.lattice_buffers(37, 29, d=30.0, jitter=1.0, layout=2, **kw)


def pair(sb, buf, tile, bounds=4000.0):
    engs = []
    for K in (0, 1):
        eng = sb.Engine(bounds_size=bounds, subticks=64, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams,
                        collision_mode=OFF, path=TILED, tile_particles=tile, block_substeps=K)
        eng.write_buffers(buf)
        engs.append(eng)
    assert engs[0].info("plan_depth") >= 7 and engs[1].info("plan_depth") == 1
    assert engs[0].info("blocked_addressing") in (FLAT, BUFFER)
    return engs


def step_and_compare(eng, ref, buf, what, calls=CALLS):
    for n in calls:
        eng.step(n)
        ref.step(n)
        assert_same(eng.load_buffers(buf.copy()), ref.load_buffers(buf.copy()), "%s, after step(%d)" % (what, n))
    assert eng.info("blocked_addressing") in (FLAT, BUFFER)
    eng.destroy()
    ref.destroy()


def test_partial_waves_and_an_almost_empty_halo_slot(sb):
    buf = lattice(sb)
    eng, ref = pair(sb, buf, 256)
    assert eng.info("tiles") >= 4
    step_and_compare(eng, ref, buf, "37 x 29, tile_particles = 256")


def test_one_tile_has_no_halo(sb):
    """ONE tile: no halo particle, no halo entry -- every request of the halo classes is out of range.  (A tile owns at most 1024
    particles, fewer than the 37 x 29 lattice has: the one tile is a 31 x 29 lattice, 899 particles, again no multiple of 64.)"""
    buf = sb.scenes.lattice_buffers(31, 29, d=30.0, origin=(300.0, 900.0), jitter=1.0, layout=2, velocity=(0.4, -1.0))
    eng, ref = pair(sb, buf, 1024)
    assert eng.info("tiles") == 1 and eng.info("halo_particles") == 0
    step_and_compare(eng, ref, buf, "31 x 29 in one tile")


def test_dead_entries_beside_live_ones(sb):
    """A knife through the lattice, then the delete pass: the entries of the cut beams are the dummy word in the owner's slots and in
    the halo copies, and the store phase carries their state through its flat branch beside range-checked neighbours."""
    buf = lattice(sb)
    eng, ref = pair(sb, buf, 256)
    shapes = sb.engine.cut_shapes(segments=[(250.0, 1300.0, 1500.0, 1450.0)])
    for e in (eng, ref):
        e.step(3)
        e.cut(shapes)
        e.delete_pass()
    got = eng.load_buffers(buf.copy())
    assert 0 < buf.beam_count - got.beam_count < buf.beam_count // 10, "the knife must remove a few beams"
    assert_same(got, ref.load_buffers(buf.copy()), "after the cut")
    step_and_compare(eng, ref, buf, "after a cut")


def test_yielded_tile_beside_pristine_ones(sb):
    """One corner particle pulled outwards: its beams yield in the first substeps, their tile stores and reads its targets from
    then on (own_plastic), the tiles around gather them (nb_plastic), the far tiles stay pristine."""
    buf = lattice(sb, velocity=(0.0, 0.0))
    buf.particles[0, 0] -= 12.0
    buf.particles[0, 1] -= 12.0
    eng, ref = pair(sb, buf, 256)
    step_and_compare(eng, ref, buf, "a stretched corner")
    # (destroyed above: the yield is checked on a fresh run of the reference engine alone)
    chk = sb.Engine(bounds_size=4000.0, subticks=64, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams,
                    collision_mode=OFF, path=TILED, tile_particles=256, block_substeps=1)
    chk.write_buffers(buf)
    chk.step(7)
    out = chk.load_buffers(buf.copy())
    chk.destroy()
    B = out.beam_count
    moved = int((out.beams["target_length"][:B] != out.beams["length"][:B]).sum())
    assert 0 < moved <= 8, "a few beams of one corner must have yielded, %d did" % moved


def test_accelerations_live_on_the_floor(sb):
    """The lattice's bottom rows meet the floor (collisions off, walls acting): accelerations are no longer zero, so the own
    acceleration loads, the halo acceleration gathers and the flat acceleration stores run beside the range-checked ones."""
    buf = lattice(sb, origin=(300.0, 12.0), velocity=(0.3, -6.0))
    eng, ref = pair(sb, buf, 256)
    step_and_compare(eng, ref, buf, "on the floor")


def test_material_mode_1(sb):
    buf = sb.scenes.rest_at_current_length(lattice(sb))
    eng, ref = pair(sb, buf, 256)
    assert eng.info("material_mode") == 1
    step_and_compare(eng, ref, buf, "rest lengths of their own")


def test_wide_word(sb):
    buf = lattice(sb)
    B = buf.beam_count
    buf.beams["spring"][:B] = (40.0 + np.arange(B) % 8).astype("f4")  # two rest lengths x eight springs, and one more row
    buf.beams["spring"][B // 2] = 70.0
    eng, ref = pair(sb, buf, 256)
    assert eng.info("materials") == 17 and eng.info("blocked_word_format") == 0
    step_and_compare(eng, ref, buf, "17 material rows")


def test_arrays_end_at_the_last_tile(sb):
    """max_particles == particle_count and max_beams == beam_count: the last lanes' offsets are the last valid ones of every array,
    and the strain / stress pass of the launches that end a call has nothing behind its arrays but its dump elements."""
    full = lattice(sb)
    P, B = full.particle_count, full.beam_count
    buf = sb.Buffers(2, P, B)
    buf.set_scene(full.particles[:P], full.beams[:B])
    assert buf.max_particles == buf.particle_count == P and buf.max_beams == buf.beam_count == B
    eng, ref = pair(sb, buf, 256)
    step_and_compare(eng, ref, buf, "arrays at capacity")
