"""BatchEngine (sb_batch_*: N small scenes, one workgroup per scene, one launch per frame) against the CPU oracle, one
oracle.OracleEngine per scene.  The bar is the project's: bit-exact, no tolerance anywhere.  Scenes, seeds and schedules live in
tests/batch_cases.py; tests/test_batch_cpu.py asserts on the CPU that the oracle stays finite on every one of them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
from batch_harness import apply_to_batch, make_batch, upload_each  # noqa: E402

pytestmark = pytest.mark.gpu


def compare_all(be, case, refs, what=""):
    for i, (buf, ref) in enumerate(zip(case["bufs"], refs)):
        if ref is None:
            continue
        got = be.load_scene(i, buf.copy())
        exp = ref.load_buffers(buf.copy())
        assert np.isfinite(exp.particles).all()
        bc.assert_same(got, exp, "%s %s: scene %d" % (case["name"], what, i))


def run_case(sb, oracle, case, every_op=False):
    """The whole program on the batch and on one oracle per scene; compared at the end (every_op: after every op as well)."""
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    refs = [None if b is None else bc.make_oracle(oracle, case, b) for b in case["bufs"]]
    for k, op in enumerate(case["program"]):
        apply_to_batch(be, op)
        bc.apply_to_oracles(refs, op)
        if every_op:
            compare_all(be, case, refs, "after op %d" % k)
    compare_all(be, case, refs)
    return be, refs


@pytest.mark.parametrize("layout", [1, 2])
def test_default_scene_replicated_over_64_scenes(sb, oracle, layout):
    case = bc.case_default(sb, layout)
    buf = case["bufs"][0]
    be = make_batch(sb, case, n=64)
    be.write_scene(buf)                      # count=None: replicated over the batch
    ref = bc.make_oracle(oracle, case, buf)
    for op in case["program"]:
        apply_to_batch(be, op)
        bc.apply_to_oracles([ref], op)
    exp = ref.load_buffers(buf.copy())
    assert not np.array_equal(exp.particles, buf.particles)
    for i in range(64):
        bc.assert_same(be.load_scene(i, buf.copy()), exp, "default v%d scene %d" % (layout, i))
    assert be.info("frames_done") == 3 and be.info("threads_per_scene") < 1024   # the default scene does not occupy 1024 lanes
    assert be.info("frame_kernel_scratch_bytes") == 0
    be.destroy()


def test_heterogeneous_batch(sb, oracle):
    """Default scene, 12 x 12 lattice, 32 x 32 jittered lattice (1024 particles: the capacity), two particles, an empty scene and
    one never uploaded, different physics constants each, 2 frames + 7 substeps (odd count, mid-frame)."""
    case = bc.case_hetero(sb)
    be, refs = run_case(sb, oracle, case)
    assert case["bufs"][2].particle_count == be.info("scene_max_particles") == 1024
    with pytest.raises(sb.EngineError) as ei:
        be.load_scene(5, case["bufs"][0].copy())
    assert ei.value.status == 5              # never uploaded
    p, b, a = be.state_tensors()
    assert bool(p[5].isnan().all()) and bool(p[4].isnan().all()) and not bool(a[4:].any())
    be.destroy()


def test_yield_break_and_delete_per_scene(sb, oracle):
    case = bc.case_break(sb)
    be, refs = run_case(sb, oracle, case, every_op=True)
    removed = [b.beam_count - int(r.metadata[6]) for b, r in zip(case["bufs"], refs)]
    assert max(removed) > 0 and min(removed) == 0, removed
    exp = refs[4].load_buffers(case["bufs"][4].copy())
    assert (exp.beams["target_length"][:exp.beam_count] != exp.beams["length"][:exp.beam_count]).any()   # plastic yield happened
    be.destroy()


def test_permuted_mapping_and_coincident_particles(sb, oracle):
    case = bc.case_mapping(sb)
    be, refs = run_case(sb, oracle, case)
    co = refs[1].load_buffers(case["bufs"][1].copy())
    assert co.particles[40, 1] != co.particles[3, 1]        # the coincident pair was separated
    be.destroy()


def test_user_input_per_scene_from_a_device_tensor(sb, oracle):
    case = bc.case_inputs(sb)
    be, refs = run_case(sb, oracle, case, every_op=True)
    a, b = (be.load_scene(i, case["bufs"][i].copy()) for i in (0, 2))
    assert not np.array_equal(a.particles, b.particles)     # the scenes did get different inputs
    be.destroy()


def test_frames_in_one_call_and_substep_granularity(sb, oracle):
    """n_frames = 3 in one call equals three calls of one; step(64) + delete_pass() equals frame()."""
    case = bc.case_break(sb)
    runs = []
    for how in ("three", "one", "steps"):
        be = make_batch(sb, case)
        upload_each(be, case["bufs"])
        if how == "three":
            be.frame(3)
        elif how == "one":
            for _ in range(3):
                be.frame()
        else:
            for _ in range(3):
                be.step(40)
                be.step(24)
                be.delete_pass()
        runs.append([be.load_scene(i, b.copy()) for i, b in enumerate(case["bufs"])])
        be.destroy()
    refs = bc.run_oracles(oracle, case)
    for i, buf in enumerate(case["bufs"]):
        exp = refs[i].load_buffers(buf.copy())
        for run, how in zip(runs, ("frame(3)", "3 x frame()", "step + delete_pass")):
            bc.assert_same(run[i], exp, "%s scene %d" % (how, i))


def test_reset_by_device_mask(sb, oracle):
    """After 2 frames the odd scenes go back to their upload (beams the delete pass removed come back), the even ones are
    untouched; 2 more frames still equal the oracle (restarted for the odd ones)."""
    import torch
    case = bc.case_break(sb)
    bufs = case["bufs"]
    be = make_batch(sb, case)
    upload_each(be, bufs)
    refs = [bc.make_oracle(oracle, case, b) for b in bufs]
    be.frame(2)
    for r in refs:
        r.frame()
        r.frame()
    assert any(int(r.metadata[6]) < b.beam_count for r, b in list(zip(refs, bufs))[1::2]), "an odd scene must have lost beams"
    before = [be.load_scene(i, b.copy()) for i, b in enumerate(bufs)]
    mask = torch.zeros(len(bufs), dtype=torch.uint8, device="cuda")
    mask[1::2] = 1
    be.reset(mask)
    fresh = make_batch(sb, case)
    upload_each(fresh, bufs)
    for i, b in enumerate(bufs):
        got = be.load_scene(i, b.copy())
        if i % 2:
            bc.assert_same(got, fresh.load_scene(i, b.copy()), "reset scene %d equals a fresh upload" % i)
            bc.assert_same(got, b, "reset scene %d equals the uploaded buffers" % i)
            refs[i] = bc.make_oracle(oracle, case, b)
        else:
            bc.assert_same(got, before[i], "scene %d untouched by the reset" % i)
    ps, bs, al = be.state_tensors()
    pf, bf, af = fresh.state_tensors()
    for i in range(1, len(bufs), 2):
        assert torch.equal(ps[i].view(torch.int32), pf[i].view(torch.int32)) and torch.equal(bs[i].view(torch.int32), bf[i].view(torch.int32))
        assert torch.equal(al[i], af[i]) and int(al[i].sum()) == bufs[i].beam_count
    fresh.destroy()
    be.frame(2)
    for r in refs:
        r.frame()
        r.frame()
    compare_all(be, case, refs, "2 frames after the reset")
    be.reset(torch.ones(len(bufs), dtype=torch.bool, device="cuda"))      # a bool mask, all scenes
    for i, b in enumerate(bufs):
        bc.assert_same(be.load_scene(i, b.copy()), b, "reset of all, scene %d" % i)
    be.destroy()


def check_state_rows(sb, be, bufs, what):
    """state_tensors() on sentinel-filled outputs: rows of a scene's particles / beams equal load_scene(i), all others keep the
    sentinel."""
    import torch
    p, b, a = (t.cpu().numpy() for t in be.state_tensors())
    for i, buf in enumerate(bufs):
        if buf is None:
            assert np.isnan(p[i]).all() and np.isnan(b[i]).all() and not a[i].any()
            continue
        got = be.load_scene(i, buf.copy())
        P, B0 = got.particle_count, buf.beam_count
        pidx = got.mapping[:P].astype(np.int64)
        assert np.array_equal(p[i][pidx].view("u4"), got.particles[pidx].view("u4")), "%s scene %d particles" % (what, i)
        rest = np.ones(be.max_particles, bool)
        rest[pidx] = False
        assert np.isnan(p[i][rest]).all()
        bidx = buf.mapping[buf.max_particles:buf.max_particles + B0].astype(np.int64)      # every beam of the upload
        rec = got.beams[bidx]
        exp = np.stack([rec["target_length"], rec["last_length"], rec["strain"], rec["stress"]], axis=1)
        assert np.array_equal(b[i][bidx].view("u4"), exp.view("u4")), "%s scene %d beams" % (what, i)
        rest = np.ones(be.max_beams, bool)
        rest[bidx] = False
        assert np.isnan(b[i][rest]).all() and not a[i][rest].any()
        live = got.mapping[got.max_particles:got.max_particles + got.beam_count].astype(np.int64)
        exp_alive = np.zeros(be.max_beams, bool)
        exp_alive[live] = True
        assert np.array_equal(a[i], exp_alive), "%s scene %d alive" % (what, i)
    assert isinstance(be.state_tensors()[2], torch.Tensor)


def test_state_io(sb, oracle):
    """Export rows equal load_scene (mid-frame included); export -> import -> continue leaves the run bit-identical; an import that
    scales velocities in some scenes equals the same edit uploaded to the oracle."""
    case = bc.case_break(sb)
    bufs = case["bufs"]
    n = len(bufs)
    be, plain = make_batch(sb, case), make_batch(sb, case)
    upload_each(be, bufs)
    upload_each(plain, bufs)
    refs = [bc.make_oracle(oracle, case, b) for b in bufs]
    check_state_rows(sb, be, bufs, "after upload")
    for x in (be, plain):
        x.frame(2)
        x.step(5)                                            # mid-frame
    for r in refs:
        r.frame()
        r.frame()
        r.step(5)
    check_state_rows(sb, be, bufs, "mid-frame")
    p, b, a = be.state_tensors()
    be.write_particles_device(p)                             # export -> import: nothing changes
    for i, buf in enumerate(bufs):
        bc.assert_same(be.load_scene(i, buf.copy()), plain.load_scene(i, buf.copy()), "export -> import, scene %d" % i)
    # scale the velocities of scenes 1 and 3 on the device; the oracle gets the same edit through its particle buffer
    edit = p.clone()
    edit[1, :, 2:4] *= 0.5
    edit[3, :, 2:4] *= -0.25
    be.write_particles_device(edit)
    for i, f in ((1, 0.5), (3, -0.25)):
        cur = refs[i].particles_b if refs[i].final_in_b else refs[i].particles_a
        cur[:, 2:4] *= np.float32(f)
    be.step(59)
    be.delete_pass()
    be.frame()
    for r in refs:
        r.step(59)
        r.delete_pass()
        r.frame()
    compare_all(be, case, refs, "after the import")
    check_state_rows(sb, be, bufs, "after the import")
    # a heterogeneous batch with an empty and a never-uploaded scene
    het = bc.case_hetero(sb)
    hb = make_batch(sb, het)
    upload_each(hb, het["bufs"])
    hb.frame()
    hb.step(3)
    check_state_rows(sb, hb, het["bufs"], "heterogeneous")
    for x in (be, plain, hb):
        x.destroy()
    assert n == len(bc.BREAK_SCALES)


def test_batch_agrees_with_the_single_engine(sb, oracle):
    """Scene i after 2 frames equals sb.Engine with its default collision mode (the spatial hash) on the same input, read back:
    the two products agree with each other, not only each with the oracle."""
    case = bc.case_break(sb)
    bufs = case["bufs"] + [fit_default(sb, case)]
    be = sb.BatchEngine(n_scenes=len(bufs), layout=1, max_particles=case["cap"][0], max_beams=case["cap"][1])
    upload_each(be, bufs)
    be.frame(2)
    for i, buf in enumerate(bufs):
        eng = sb.Engine(layout=1, max_particles=buf.max_particles, max_beams=buf.max_beams)      # collision_mode GRID: the default
        eng.write_buffers(buf)
        eng.frame()
        eng.frame()
        exp = eng.load_buffers(buf.copy())
        eng.destroy()
        bc.assert_same(be.load_scene(i, buf.copy()), exp, "batch vs Engine, scene %d" % i)
    be.destroy()


def fit_default(sb, case):
    return bc.fit(sb, sb.scenes.default_buffers(1, 128, 320), *case["cap"])


def test_scene_result_is_independent_of_batch_size_and_position(sb, oracle):
    """Batch of 1 against scene 37 of 300 (a count that divides neither by the 8 XCDs nor by the 256 CUs), every other scene
    a different one."""
    case = bc.case_break(sb)
    mine, other = fit_default(sb, case), case["bufs"][4]
    one = make_batch(sb, case, n=1)
    one.write_scene(mine)
    many = make_batch(sb, case, n=300)
    many.write_scene(other)
    many.write_scene(mine, 37, 1)
    ref = bc.make_oracle(oracle, case, mine)
    ref_other = bc.make_oracle(oracle, case, other)
    for x in (one, many):
        x.frame(2)
        x.step(5)
    for r in (ref, ref_other):
        r.frame()
        r.frame()
        r.step(5)
    exp = ref.load_buffers(mine.copy())
    a, b = one.load_scene(0, mine.copy()), many.load_scene(37, mine.copy())
    bc.assert_same(a, exp, "batch of 1")
    bc.assert_same(b, exp, "scene 37 of 300")
    bc.assert_same(a, b, "1 vs 300")
    exp_other = ref_other.load_buffers(other.copy())
    for i in (0, 36, 38, 255, 256, 299):
        bc.assert_same(many.load_scene(i, other.copy()), exp_other, "scene %d of 300" % i)
    one.destroy()
    many.destroy()


def test_force_saturation_in_one_scene_leaves_its_neighbours_alone(sb, oracle):
    case = bc.case_saturation(sb)
    be, refs = run_case(sb, oracle, case)
    exp = refs[1].load_buffers(case["bufs"][1].copy())
    assert np.abs(exp.particles[:4, 2:4]).max() == np.float32(32768.0 / 64.0)      # (2^31 / 65536) * dt: the saturated force
    # the neighbours equal what they compute in a batch of their own
    for i in (0, 2):
        alone = make_batch(sb, case, n=1)
        alone.write_scene(case["bufs"][i])
        alone.step(1)
        bc.assert_same(be.load_scene(i, case["bufs"][i].copy()), alone.load_scene(0, case["bufs"][i].copy()), "neighbour %d" % i)
        alone.destroy()
    be.destroy()


def test_upload_validation_and_call_errors(sb):
    case = bc.case_default(sb, 1)
    be = make_batch(sb, case, n=3)
    bad = sb.Buffers(1, 128, 320)
    beams = np.zeros(1, sb.layout.BEAM_DTYPE[1])
    beams[0]["a"], beams[0]["b"], beams[0]["length"] = 0, 9, 10.0     # endpoint 9 is not an active particle
    bad.set_scene(np.zeros((2, 6), "f4"), beams)
    with pytest.raises(sb.EngineError) as ei:
        be.write_scene(bad)
    assert ei.value.status == 1 and "references particle" in str(ei.value)
    two = sb.Buffers(1, 128, 320)
    two.set_scene(np.zeros((2, 6), "f4"), np.zeros(0, sb.layout.BEAM_DTYPE[1]))
    two.mapping[1] = 0                                                 # two slots on one data index
    with pytest.raises(sb.EngineError, match="two slots"):
        be.write_scene(two)
    with pytest.raises(sb.EngineError):
        be.write_scene(sb.Buffers(1, 64, 320))                         # another capacity
    with pytest.raises(sb.EngineError):
        be.write_scene(case["bufs"][0], 2, 2)                          # past the end of the batch
    be.frame()                                                         # nothing uploaded: a no-op
    be.sync()
    assert be.info("n_scenes") == 3 and be.info("lds_bytes_per_scene") > 0 and be.info("scenes_per_cu") >= 1
    be.destroy()


def test_kernel_resource_info_in_either_order(sb):
    """*_kernel_vgprs / *_kernel_scratch_bytes of the five kernels that are asked on demand: one batch is asked for the registers
    first, the other for the scratch bytes first, each key twice; every answer for a key is the same, the registers > 0, the
    scratch bytes 0.  Nothing is launched."""
    cap = (8, 8)
    case = dict(name="two particles twice", layout=1, cap=cap, mode=bc.OFF, bufs=[bc.two_particles(sb, 1, cap)] * 2)
    a, b = make_batch(sb, case), make_batch(sb, case)
    for be in (a, b):
        upload_each(be, case["bufs"])
    for prefix in ("render", "summary", "bodies", "contacts", "body_summary"):
        vgprs, scratch = prefix + "_kernel_vgprs", prefix + "_kernel_scratch_bytes"
        got = {vgprs: [], scratch: []}
        for be, keys in ((a, (vgprs, scratch)), (b, (scratch, vgprs))):
            for key in keys + keys:
                got[key].append(be.info(key))
        assert len(got[vgprs]) == len(got[scratch]) == 4
        assert len(set(got[vgprs])) == 1 and got[vgprs][0] > 0, (prefix, got)
        assert got[scratch] == [0, 0, 0, 0], (prefix, got)
    a.destroy()
    b.destroy()
