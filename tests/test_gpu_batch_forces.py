"""BatchEngine.forces (sb_batch_forces_device) against tests/batch_forces_ref.py, the numpy float32 restatement of
include/softbody.h's definition, on what load_scene returns; and against one oracle substep.  Every comparison is exact, floats as
uint32 words (a NaN as one word: batch_forces_ref.words).  Scenes live in tests/batch_forces_cases.py;
tests/test_batch_forces_cpu.py shows on the CPU that they bite."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
from batch_harness import load_all, make_batch, upload_each  # noqa: E402
import batch_forces_cases as fc  # noqa: E402
import batch_forces_ref as fr  # noqa: E402
from test_gpu_batch_bodies import assert_scenes_equal  # noqa: E402

pytestmark = pytest.mark.gpu

OFF, ALLPAIRS, GRID = 0, 1, 2
NAMES = ("rows", "beam_i32", "tension", "counts")
SENTINEL = -7


def batch_of(sb, case, mode=None, grid_min_particles=None):
    be = make_batch(sb, case, mode=mode, grid_min_particles=case.get("grid_min_particles") if grid_min_particles is None else grid_min_particles)
    upload_each(be, case["bufs"])
    return be


def forces_np(be, **kw):
    f = be.forces(rows=True, beam_i32=True, tension=True, counts=True, **kw)
    return tuple(x.cpu().numpy() for x in f)


def assert_forces(got, exp, what):
    for name, g, e in zip(NAMES, got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape, (what, name, g.dtype, g.shape, e.shape)
        gw, ew = fr.words(g), fr.words(e)
        if not np.array_equal(gw, ew):
            at = tuple(int(x[0]) for x in np.nonzero(gw != ew))
            raise AssertionError("%s: %s differ in %d words, first at %s: got %r, expected %r" % (what, name, int((gw != ew).sum()), at, g[at], e[at]))


def reference_now(be, case, labels=None, other_body=False):
    return fr.forces_of(load_all(be, case["bufs"]), be.max_particles, be.max_beams, case.get("radius", 10.0), case.get("subticks", 64), labels, other_body)


def check(sb, case, **kw):
    be = batch_of(sb, case, **kw)
    got = forces_np(be)
    assert_forces(got, reference_now(be, case), case["name"])
    be.destroy()
    return got


# ---------------------------------------------------------------- beams
@pytest.mark.parametrize("which", ["small", "beams"])
def test_beam_cases(sb, which):
    case = getattr(fc, "case_" + which)(sb)
    rows, beam_i32, tension, counts = check(sb, case)
    if which == "beams":
        centre = int(case["bufs"][3].mapping[0])
        assert beam_i32[3, centre, 0] == -64 and counts[4].tolist() == [6, 3, 2, 1]      # 64 saturated words wrapped; the NaN beam
        assert beam_i32[4, 4].tolist() == [2 ** 31 - 1, 0] and beam_i32[4, 5].tolist() == [-2 ** 31, 0] and np.isnan(tension[4, 1])
        assert tension[0, 0] == -21.0 and rows[0, 5, 0] == 21.0


@pytest.mark.parametrize("cap,in_lds", list(zip(fc.MATERIAL_CAPS, (1, 0))))
def test_material_rows_on_either_side_of_the_lds_limit(sb, cap, in_lds):
    case = fc.case_materials(sb, cap)
    be = batch_of(sb, case)
    assert be.info("materials_in_lds") == in_lds
    be.step(3)                                  # (a state with velocities, yielded targets and last_length != length)
    got = forces_np(be)
    assert_forces(got, reference_now(be, case), case["name"])
    assert got[3][0, :2].tolist() == [119, 299] and np.count_nonzero(got[2][0]) == 299 and len(np.unique(got[2][0])) > 6
    be.destroy()


# ---------------------------------------------------------------- liveness
def test_cut_welded_and_spawned_things_are_seen_until_they_go(sb):
    import torch
    case = fc.case_materials(sb, (128, 320))
    be = batch_of(sb, case)
    be.step(2)
    before = forces_np(be)
    hit, counts = be.cut(sb.engine.cut_shapes(discs=[(50.0, 150.0, 60.0)])[None], hit=True)
    flagged = hit[0].cpu().numpy().astype(bool)
    assert flagged.sum() > 0
    pending = forces_np(be)
    assert_forces(pending, before, "a pending flag still pulls")               # nothing but the flags changed
    assert (pending[2][0, flagged] != 0).all()
    be.frame(1)
    gone = forces_np(be)
    assert_forces(gone, reference_now(be, case), "after the delete pass")
    assert not gone[2][0, flagged].any() and gone[3][0, 1] <= 299 - flagged.sum()
    # a spawned particle and a beam welded onto it
    rows = sb.batch.new_particle_rows(torch.tensor([[[900.0, 500.0]]], device="cuda"))
    res, _ = be.add_particles(rows)
    new_p = int(res[0, 0])
    assert new_p >= 0
    weld = sb.batch.new_beam_rows(torch.tensor([[[new_p, 0]]], device="cuda", dtype=torch.int32), 5.0, 10.0, 5.0, 50.0, length=100.0)
    wres, _ = be.add_beams(weld)
    new_b = int(wres[0, 0])
    assert new_b >= 0
    grown = forces_np(be)
    assert_forces(grown, reference_now(be, case), "spawned and welded")
    assert grown[3][0, 0] == 120 and grown[2][0, new_b] != 0 and grown[0][0, new_p, :2].any()
    be.reset()
    back = forces_np(be)
    assert_forces(back, reference_now(be, case), "after reset")
    assert back[3][0, :2].tolist() == [119, 299] and back[2][0, new_b] == 0 and not fr.words(back[0][0, new_p]).any()
    be.destroy()


# ---------------------------------------------------------------- contacts
@pytest.mark.parametrize("subticks", [64, 60])
def test_contact_cases(sb, subticks):
    case = fc.case_contacts(sb, subticks)
    rows = check(sb, case)[0]
    d = case["bufs"][0].mapping[:16].astype(int)
    assert rows[0, d[6], 7] == 0 and rows[0, d[8], 7] == 1 and rows[0, d[0], 7] == 5          # exactly 2r; an ulp closer; five partners
    assert rows[0, d[14]].tolist()[2:] == [0, 0, 0, 0, 20.0, 1.0]                             # on one spot


def test_rings_of_zero_to_nine_partners(sb):
    import batch_grid_cases as gc
    case = fc.case_rings(sb)
    rows = check(sb, case)[0]
    for n, ((k, crowded), buf) in enumerate(zip(gc.ring_scenes(), case["bufs"])):
        assert rows[n, int(buf.mapping[gc.ring_points(k, crowded, n)[1]]), 7] == k, (n, k)
    walked = check(sb, case, grid_min_particles=0xFFFFFFFF)[0]
    assert np.array_equal(fr.words(walked), fr.words(rows))


def test_every_collision_mode_and_threshold_gives_the_same_words(sb):
    case = fc.case_contacts(sb)
    outs = []
    for mode, gmp in ((OFF, None), (ALLPAIRS, None), (GRID, None), (GRID, 1), (GRID, 0xFFFFFFFF), (GRID, 17)):
        be = batch_of(sb, case, mode=mode, grid_min_particles=gmp)
        outs.append(forces_np(be))
        be.destroy()
    for o in outs[1:]:
        assert_forces(o, outs[0], "another mode")
    be = batch_of(sb, case)
    assert_forces(outs[0], reference_now(be, case), "the first mode")
    be.destroy()


# ---------------------------------------------------------------- labels
def test_other_body_takes_only_the_partners_of_another_label(sb):
    import torch
    case = fc.case_two_bodies(sb)
    be = batch_of(sb, case)
    labels = be.bodies()[0]
    lab = labels.cpu().numpy()
    every = forces_np(be, labels=True)
    cross = forces_np(be, labels=True, other_body=True)
    assert_forces(every, reference_now(be, case), "labels without the flag change nothing")
    assert_forces(cross, reference_now(be, case, lab, True), "other_body with bodies()' labels")
    assert every[0][0, :, 7].sum() == 44 and cross[0][0, :, 7].sum() == 6 and cross[3][0, 2] == 6 and every[3][0, 2] == 15
    assert_forces(cross[1:3], every[1:3], "the beam part does not look at labels")
    own = torch.full((2, be.max_particles), -123456789, dtype=torch.int32, device="cuda")     # a partition of the caller's own
    own[0, ::2] = 2 ** 31 - 1
    assert_forces(forces_np(be, labels=own, other_body=True), reference_now(be, case, own.cpu().numpy(), True), "the caller's labels")
    with pytest.raises(sb.EngineError) as ei:
        be.forces(other_body=True)
    assert ei.value.status == 1 and "labels" in str(ei.value)
    be.destroy()


# ---------------------------------------------------------------- read-only
def test_forces_only_read(sb):
    case = bc.case_break(sb)
    a, b = make_batch(sb, case), make_batch(sb, case)
    for be in (a, b):
        upload_each(be, case["bufs"])
    state = [x.clone() for x in a.state_tensors()]
    scenes = [s.particles.tobytes() + s.beams.tobytes() + s.mapping.tobytes() + s.metadata.tobytes() for s in load_all(a, case["bufs"])]
    a.forces(labels=True, other_body=True, beam_i32=True, tension=True, counts=True)
    for x, y in zip(state, a.state_tensors()):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    assert scenes == [s.particles.tobytes() + s.beams.tobytes() + s.mapping.tobytes() + s.metadata.tobytes() for s in load_all(a, case["bufs"])]
    for k in range(3):
        a.frame(1)
        b.frame(1)
        a.forces(tension=True, counts=True)
        a.step(3)
        b.step(3)
        a.forces(labels=True)
    assert_scenes_equal(a, b, case["bufs"], "three frames with forces() in between")
    assert a.info("substeps_done") == b.info("substeps_done")
    a.destroy()
    b.destroy()


# ---------------------------------------------------------------- the oracle anchor
@pytest.mark.parametrize("name", ["beams only", "contacts only", "both"])
def test_one_substep_of_the_batch_and_of_the_oracle_are_the_forces(sb, oracle, name):
    case = fc.case_anchor(sb, name)
    buf = case["bufs"][0]
    be = batch_of(sb, case)
    rows, _, tension, _ = forces_np(be)
    be.step(1)
    got = load_all(be, case["bufs"])[0]
    ref = oracle.OracleEngine(1000.0, 10.0, 64, buf.layout, oracle.COLLIDE_ALLPAIRS)
    ref.write_buffers(buf)
    ref.step(1)
    bc.assert_same(got, ref.load_buffers(buf.copy()), name)
    idx = buf.mapping[:buf.particle_count].astype(int)
    want_v = (rows[0, idx, 2:4] + rows[0, idx, 0:2]) * np.float32(2.0 ** -6)
    assert np.abs(want_v).max() > 0 and np.array_equal(fr.words(got.particles[idx, 2:4]), fr.words(want_v))
    bd = buf.mapping[buf.max_particles:buf.max_particles + buf.beam_count].astype(int)
    assert np.array_equal(fr.words(got.beams["stress"][bd]), fr.words(tension[0, bd] * fr.STRESS_SCALE))
    be.destroy()


# ---------------------------------------------------------------- rows and masks
def test_mixed_scenes_sentinels_and_every_combination_of_outputs(sb):
    import torch
    case = fc.case_mixed(sb)
    n, (maxP, maxB) = len(case["bufs"]), case["cap"]
    be = batch_of(sb, case)
    be.step(2)
    exp = reference_now(be, case)
    assert exp[3][:, 0].tolist()[:5] == [119, 0, 64, 0, 2] and len(set(exp[3][:, 0].tolist())) >= 8
    assert not any(fr.words(x[[1, 3]]).any() for x in exp)                     # never uploaded, empty: zeros
    shapes = ((n + 1, maxP, 8), (n + 1, maxP, 2), (n + 1, maxB), (n + 1, 4))
    dtypes = (torch.float32, torch.int32, torch.float32, torch.int32)
    L = sb.batch.load_library()
    for mask in (1, 2, 4, 8, 5, 10, 15):
        outs = [torch.full(s, SENTINEL, dtype=t, device="cuda") for s, t in zip(shapes, dtypes)]
        torch.cuda.synchronize()
        ptrs = [ctypes.c_void_p(o.data_ptr()) if mask >> k & 1 else None for k, o in enumerate(outs)]
        assert L.sb_batch_forces_device(be._h, 0, None, *ptrs) == 0, L.sb_batch_last_error(be._h)
        be.sync()
        for k, o in enumerate(outs):
            a = o.cpu().numpy()
            if mask >> k & 1:
                assert np.array_equal(fr.words(a[:n]), fr.words(exp[k])) and (a[n:] == SENTINEL).all(), (mask, NAMES[k])
            else:
                assert (a == SENTINEL).all(), (mask, NAMES[k])
    # a rows buffer that is only 4-byte aligned; all outputs NULL
    raw = torch.full((n * maxP * 8 + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert L.sb_batch_forces_device(be._h, 0, None, ctypes.c_void_p(raw.data_ptr() + 4), None, None, None) == 0
    assert L.sb_batch_forces_device(be._h, 0, None, None, None, None, None) == 0
    be.sync()
    a = raw.cpu().numpy()
    assert a[0] == SENTINEL and a[-3:].tolist() == [SENTINEL] * 3 and np.array_equal(fr.words(a[1:1 + n * maxP * 8].reshape(n, maxP, 8)), fr.words(exp[0]))
    # the Python call: each output as None
    f = be.forces()
    assert f.beam_i32 is None and f.tension is None and f.counts is None and np.array_equal(fr.words(f.rows.cpu().numpy()), fr.words(exp[0]))
    f = be.forces(rows=None, tension=True)
    assert f.rows is None and f.counts is None and np.array_equal(fr.words(f.tension.cpu().numpy()), fr.words(exp[2]))
    mine = torch.full((n, 4), SENTINEL, dtype=torch.int32, device="cuda")
    f = be.forces(rows=False, counts=mine, beam_i32=True)
    assert f.counts is mine and np.array_equal(mine.cpu().numpy(), exp[3]) and np.array_equal(f.beam_i32.cpu().numpy(), exp[1])
    # determinism
    assert_forces(forces_np(be), forces_np(be), "two calls")
    be.destroy()


def test_argument_errors(sb):
    import torch
    case = fc.case_small(sb)
    be = batch_of(sb, case)
    L = sb.batch.load_library()
    vp = ctypes.c_void_p
    p = torch.zeros(4 * 8 * 8 + 8, dtype=torch.int32, device="cuda").data_ptr()
    for args, needle in (((None, 0, None, vp(p), None, None, None), "null batch"), ((be._h, 2, None, vp(p), None, None, None), "flags 0x2"),
                         ((be._h, 0x80000001, vp(p), vp(p), None, None, None), "flags 0x80000001"), ((be._h, 1, None, vp(p), None, None, None), "labels"),
                         ((be._h, 0, vp(p + 2), vp(p), None, None, None), "4-byte aligned"), ((be._h, 0, None, vp(p + 1), None, None, None), "4-byte aligned"),
                         ((be._h, 0, None, None, vp(p + 3), None, None), "4-byte aligned"), ((be._h, 0, None, None, None, vp(p + 2), None), "4-byte aligned"),
                         ((be._h, 0, None, None, None, None, vp(p + 1)), "4-byte aligned")):
        assert L.sb_batch_forces_device(*args) == 1, needle
        msg = L.sb_batch_last_error(args[0]).decode()
        assert "sb_batch_forces_device" in msg and needle in msg, (needle, msg)
    for call in (lambda: be.forces(rows=torch.zeros((4, 8, 8), dtype=torch.int32, device="cuda")), lambda: be.forces(rows=torch.zeros((4, 8, 8))),
                 lambda: be.forces(tension=torch.zeros((4, 7), device="cuda")), lambda: be.forces(labels="yes"), lambda: be.forces(counts="no")):
        with pytest.raises(ValueError):
            call()
    assert 0 < be.info("forces_kernel_vgprs") <= 128 and be.info("forces_kernel_scratch_bytes") == 0 and be.info("force_words") == 8
    assert be.forces(counts=True).counts.cpu().numpy()[:, 0].tolist() == [2, 6, 6, 6]
    be.destroy()


# ---------------------------------------------------------------- full width, once
def test_full_width(sb):
    case = fc.case_full_width(sb)
    got = check(sb, case)
    assert got[3][:, 0].tolist() == [1024, 1024] and (got[3][:, 2] > 900).all() and (got[0][..., 7] >= 4).sum() > 100
