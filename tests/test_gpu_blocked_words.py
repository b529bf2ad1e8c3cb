"""The blocked kernel's LDS planes and the two forms it holds its entry words in (csrc/sb_blocked_word.h): positions and force
sums lie in four planes behind one byte offset per endpoint, and a scene with at most 16 material rows has its words repacked
once per launch into those byte offsets ("narrow", sb_get_info blocked_word_format = 1); more rows keep the word as it lies in
HBM ("wide", 0).  Bit for bit against the oracle -- particles, beam target / last length, strain / stress of the last substep of a
call, the counts -- at the smallest shapes that reach every user of the layout and both forms: several tiles with halos and
padding slots at launch depths 1, 3 and 7, exactly 16 and 17 rows, material mode 1 (wide on the planes; under the spatial hash
wide on the record layout), dead entries after a delete pass, regions past 2048 records and the regions a lowered depth leaves,
the tracked variants under the spatial hash, the general particle phase."""
import numpy as np
import pytest

from test_gpu_parity import GRID, OFF, TILED, assert_same

pytestmark = pytest.mark.gpu
NARROW, WIDE = 1, 0


def lattice40(sb, **kw):
    return sb.scenes.lattice_buffers(40, 40, d=30.0, origin=(300.0, 900.0), jitter=1.0, layout=2, velocity=(0.4, -1.0), **kw)


def with_rows(sb, buf, rows):
    """Per-beam springs that bring the material dictionary to exactly `rows` rows: the lattice has two rest lengths, each gets
    rows // 2 springs, and for an odd count one beam more gets a spring of its own."""
    B = buf.beam_count
    lengths = np.unique(buf.beams["length"][:B])
    assert lengths.size == 2 and rows >= 2
    buf.beams["spring"][:B] = (40.0 + np.arange(B) % (rows // 2)).astype("f4")
    if rows % 2:
        buf.beams["spring"][B // 2] = 70.0
    return buf


def engines(sb, oracle, buf, *, K=0, tile=256, bounds=4000.0, mode=OFF):
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


# Depths 1, 3 and 7 are depths of a LAUNCH: with a plan depth the caller names a call runs in the fewest launches, so step(1),
# step(3) and step(7) are ONE launch of that depth, the strain / stress variant; 37 and 15 are odd counts no depth divides (lean
# launches, then a strain / stress launch).  There is no PLAN of depth 1 to add: block_substeps=1 asks for the single-substep
# kernel (sb_options in include/softbody.h), and the blocked kernel reaches one substep a launch only as such a short launch.
@pytest.mark.parametrize("K,calls", [(7, (1, 3, 7, 15)), (3, (1, 3, 37))])
def test_narrow_words_on_several_tiles(sb, oracle, K, calls):
    buf = lattice40(sb)
    eng, ref = engines(sb, oracle, buf, K=K)
    assert eng.info("tiles") >= 4 and eng.info("plan_depth") == K and eng.info("materials") == 2
    assert eng.info("blocked_word_format") == NARROW
    step_and_compare(eng, ref, buf, calls, "40 x 40, K = %d" % K)
    eng.destroy()


@pytest.mark.parametrize("rows,form", [(16, NARROW), (17, WIDE)])
def test_sixteen_rows_are_narrow_and_seventeen_wide(sb, oracle, rows, form):
    buf = with_rows(sb, lattice40(sb), rows)
    eng, ref = engines(sb, oracle, buf, K=7)
    assert eng.info("material_mode") == 2 and eng.info("materials") == rows and eng.info("plan_depth") == 7
    assert eng.info("blocked_word_format") == form
    step_and_compare(eng, ref, buf, (1, 3, 7, 15), "%d rows" % rows)
    eng.destroy()


def test_material_mode_1_stays_wide_on_the_planes(sb, oracle):
    """Rest lengths of their own per beam: the rows hold spring, damp, yield and limit only, the lengths come from LDS (s_len).
    The mode-1 variants keep the wide word (their narrow forms spill registers where the wide ones do not, so the engine does
    not pick them: csrc/sb_blocked.hip sbk_word_format); positions and sums still go through the planes."""
    buf = sb.scenes.rest_at_current_length(lattice40(sb))
    eng, ref = engines(sb, oracle, buf, K=7)
    assert eng.info("material_mode") == 1 and eng.info("plan_depth") == 7
    assert eng.info("blocked_word_format") == WIDE
    step_and_compare(eng, ref, buf, (1, 3, 7, 15), "material mode 1")
    eng.destroy()


@pytest.mark.parametrize("rows,form", [(2, NARROW), (17, WIDE)])
def test_dead_entries_after_a_delete_pass(sb, oracle, rows, form):
    """A 15 x 12 lattice thrown into the corner, cut into small tiles that hold copies of each other's beams: beams yield (their
    targets are stored), cross their break limit and are removed by the delete pass of a frame -- their entries are the dummy
    word from then on, which the strain / stress pass and the store phase must still recognise; then more substeps."""
    buf = sb.scenes.lattice_buffers(15, 12, d=30.0, origin=(30.0, 30.0), spring=50.0, damp=100.0, yield_strain=0.05, strain_limit=0.12,
                                    layout=1, velocity=(-40.0, -35.0), slack=8)
    if rows != 2:
        B = buf.beam_count
        buf.beams["damp"][:B] = (100.0 + np.arange(B) % (rows // 2)).astype("f4")
        buf.beams["damp"][B // 2] = 90.0
    eng, ref = engines(sb, oracle, buf, K=3, tile=64, bounds=1000.0)
    assert eng.info("materials") == rows and eng.info("blocked_word_format") == form
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


def test_region_indices_past_2048(sb, oracle):
    """Endpoints whose region index sets the top bit of a narrow word's 14-bit fields (4 x 2048 = 2^13) in real entries, not only
    in the dummy and padding records from 2560 on.  What stops a region short of that on the lattices above is the kernel's 3072
    halo ENTRIES, three or four per halo particle; a square grid of axial beams alone has two, so full 1024-particle tiles
    (32 x 32) keep a depth of 8 with more than a thousand halo particles around an inner tile."""
    full = sb.scenes.lattice_buffers(128, 128, d=25.0, origin=(100.0, 100.0), jitter=1.0, layout=2, strain_limit=1e9, velocity=(0.4, -1.0))
    P, B = full.particle_count, full.beam_count
    axial = full.beams[:B][full.beams["length"][:B] == np.float32(25.0)]
    assert 0 < len(axial) < B
    buf = sb.Buffers(2, P, len(axial))
    buf.set_scene(full.particles[:P], axial)
    eng, ref = engines(sb, oracle, buf, K=8, tile=1024, bounds=4000.0)
    assert eng.info("plan_depth") == 8 and eng.info("substeps_per_launch") == 8 and 2048 < eng.info("region_particles") <= 2560
    assert eng.info("materials") == 1 and eng.info("blocked_word_format") == NARROW
    step_and_compare(eng, ref, buf, (8, 11), "axial grid, regions past 2048")
    eng.destroy()


def test_large_regions_of_a_lowered_depth(sb, oracle):
    """K = 8 on 700-particle tiles of a 4-beam lattice is lowered until the halo fits the kernel's slots (to 6, the plan's regions
    reach 1826 particles at depth 8): halo endpoints far past the 1024 own records at a depth the engine chose itself."""
    buf = sb.scenes.lattice_buffers(96, 96, d=25.0, origin=(100.0, 100.0), anti_diagonal=True, jitter=1.0, layout=2, strain_limit=1e9)
    eng, ref = engines(sb, oracle, buf, K=8, tile=700)
    assert 1 < eng.info("plan_depth") < 8 and 1024 < eng.info("region_particles") <= 2560
    assert eng.info("blocked_word_format") == NARROW
    step_and_compare(eng, ref, buf, (7, 12), "lowered K")
    eng.destroy()


@pytest.mark.parametrize("rows,form", [(2, NARROW), (17, WIDE), (0, WIDE)])
def test_tracked_variants_under_the_spatial_hash(sb, oracle, rows, form):
    """Nothing is within reach of anything: after the stretch of single substeps that builds the hash the calls run as tracked
    blocked launches.  rows = 0: rest lengths of their own (material mode 1) -- the tracked mode-1 variants keep the record
    layout of LDS (csrc/sb_blocked.hip SbLdsRecords)."""
    buf = lattice40(sb)
    if rows == 0:
        sb.scenes.rest_at_current_length(buf)
    elif rows != 2:
        with_rows(sb, buf, rows)
    eng, ref = engines(sb, oracle, buf, mode=GRID, bounds=6000.0, tile=0)
    step_and_compare(eng, ref, buf, (1, 7, 13, 100), "40 x 40, spatial hash, %d rows" % rows)
    assert eng.info("material_mode") == (1 if rows == 0 else 2)
    assert eng.info("hybrid_substeps") > 0 and eng.info("blocked_word_format") == form
    eng.destroy()


@pytest.mark.parametrize("rows,form", [(2, NARROW), (17, WIDE)])
def test_general_particle_phase(sb, oracle, rows, form):
    """A drag exponent that is not 2 and user input: the variants with the particle phase spelled out."""
    buf = lattice40(sb)
    if rows != 2:
        with_rows(sb, buf, rows)
    buf.user_strength = 1.5
    eng, ref = engines(sb, oracle, buf, K=7)
    b = buf.copy()
    b.set_user_input(applied_force=(0.3, 0.1), mouse_pos=(600.0, 1200.0), mouse_vel=(4.0, 2.0), mouse_active=True)
    for e in (eng, ref):
        e.write_user_input(b.user_input_bytes())
        e.set_physics_constants(np.array([0.1, -0.8, 0.4, 0.3, 0.6, 0.2, 0.002, 2.5], "f4"))
    assert eng.info("blocked_word_format") == form
    step_and_compare(eng, ref, buf, (1, 3, 7, 15), "drag exponent 2.5, %d rows" % rows)
    eng.destroy()
