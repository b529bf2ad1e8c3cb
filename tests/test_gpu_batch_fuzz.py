"""Seeded fuzzing of the batch's frame kernel (k_batch_frame) against one all-pairs OracleEngine per scene:
capacities that are no whole waves or flag words and that sit on either side of "the material rows fit the LDS", bounds, radius
and subticks other than 1000 / 10 / 64 (63 is rounded up, 48 and 100 take the division by dt^2), all three collision modes and
every threshold of the contact cells, sparse shuffled mappings, per-scene constants and user input, programs of frames, odd and
even substep runs, delete passes and changed constants and inputs.  After EVERY op every uploaded scene is compared with
batch_cases.assert_same: bit for bit, no tolerance.  Cases: tests/batch_fuzz_cases.py; tests/test_batch_fuzz_cpu.py shows without a
GPU that they stay finite and that they bite.  SB_FUZZ_OFFSET / SB_FUZZ_COUNT shift and widen the seeds (a soak)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
import batch_fuzz_cases as fz  # noqa: E402
from batch_harness import apply_to_batch, make_batch, upload_each  # noqa: E402

pytestmark = pytest.mark.gpu

RAN = {}                         # seed -> (variant the batch reported, cell_substeps, cell_overflow_substeps)


@pytest.mark.parametrize("seed", range(fz.SEED0, fz.SEED0 + fz.COUNT))
def test_random_batch_equals_oracle(sb, oracle, seed):
    case = fz.case(sb, seed)
    bufs, exp = case["bufs"], case["expect"]
    be = make_batch(sb, case, mode=case["mode"], grid_min_particles=case["grid_min_particles"])
    assert be.subticks == (case["subticks"] + 1) // 2 * 2
    # what the batch says about itself is what the restated formulas say
    assert be.info("materials_in_lds") == int(exp["materials_in_lds"])
    assert be.info("threads_per_scene") == exp["threads"]
    assert be.info("lds_bytes_per_scene") == exp["lds_bytes"]
    assert be.info("contact_cells_per_side") == exp["cells_per_side"]
    assert be.info("grid_min_particles") == exp["grid_min_particles"]
    assert be.info("frame_kernel_scratch_bytes") == 0
    upload_each(be, bufs)
    refs = [None if b is None else fz.make_oracle(oracle, case, b) for b in bufs]
    for k, op in enumerate(case["program"]):
        apply_to_batch(be, op)
        bc.apply_to_oracles(refs, op)
        for i, (buf, ref) in enumerate(zip(bufs, refs)):
            what = "seed %d, scene %d (%s) after op %d %s" % (seed, i, case["kinds"][i], k, op[:2])
            if ref is None:
                with pytest.raises(sb.EngineError) as ei:
                    be.load_scene(i, bufs[case["empty"]].copy())
                assert ei.value.status == 5, what                # never uploaded
                continue
            want = ref.load_buffers(buf.copy())
            assert np.isfinite(fz.live_particles(ref)).all(), what + ": the oracle is not finite (the generator drifted)"
            got = be.load_scene(i, buf.copy())
            bc.assert_same(got, want, what)
            if i == case["empty"]:
                assert (got.particle_count, got.beam_count) == (0, 0), what
    collide = fz.NONE if case["mode"] == fz.OFF else fz.CELLS if be.info("contact_cells_per_side") else fz.WALK
    on_cells, fell_back = be.info("cell_substeps"), be.info("cell_overflow_substeps")
    assert (collide, bool(be.info("materials_in_lds"))) == case["expect_variant"]
    st = be.subticks
    n_sub = sum(op[1] * st if op[0] == "frame" else op[1] if op[0] == "step" else 0 for op in case["program"])
    assert on_cells + fell_back == n_sub * sum(fz.takes_cells(case, i) for i in range(len(bufs)))
    RAN[seed] = (case["expect_variant"], on_cells, fell_back)
    be.destroy()


def test_the_family_ran_every_variant_on_and_off_the_cells():
    """(after the cases above) all six instances of the kernel ran; scenes stepped on the cells and fell back to the walk, both
    within single cases"""
    if not RAN:
        pytest.skip("the batch fuzz cases did not run in this session")
    variants = {v[0] for v in RAN.values()}
    on_cells, fell_back = sum(v[1] for v in RAN.values()), sum(v[2] for v in RAN.values())
    both = sum(1 for v in RAN.values() if v[1] > 0 and v[2] > 0)
    print("batch fuzz: %d cases, variants %s, %d scene-substeps on the cells, %d fell back, both in %d cases"
          % (len(RAN), sorted(variants), on_cells, fell_back, both))
    if len(RAN) >= fz.NSEEDS:                                    # (a selection of a few seeds only reports)
        assert on_cells > 0 and fell_back > 0
    if set(range(fz.NSEEDS)) <= set(RAN):                        # the committed seeds: tests/test_batch_fuzz_cpu.py shows that they can
        assert variants == set(fz.VARIANTS) and both >= 3
