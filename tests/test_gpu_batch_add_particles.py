"""BatchEngine.add_particles (sb_batch_add_particles_device) on the GPU, every comparison bit for bit: the edit equals
tests/batch_add_particles_ref.py on what load_scene returns; the frames after equal the oracle started from the edited scene;
adding on the device equals uploading the edited scene; every row code and the 2r boundary; room; which index a new particle
gets; reset, checkpoint, fork and masks around an add; a dry run; what later calls see; add_particles -> body_beam_rows ->
add_beams spawns a body."""
import numpy as np
import pytest

import batch_add_beams_ref as beam_ref
import batch_add_particles_cases as cases
import batch_add_particles_ref as ref
import batch_contacts_ref
from batch_harness import load_all, make_batch, upload_each
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

OFF, ALLPAIRS, GRID = 0, 1, 2
E, I, B, FULL = ref.EMPTY, ref.INVALID, ref.BLOCKED, ref.FULL


def dev(a, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()


def batch(sb, case, mode=OFF, **kw):
    case = dict(case, mode=mode)
    be = make_batch(sb, case, mode=mode, **kw)
    upload_each(be, case["bufs"])
    return be


def add(be, rows, flags=0, dry=False):
    res, cnt = be.add_particles(dev(rows), skip_touching=bool(flags & ref.SKIP_TOUCHING), dry_run=dry)
    return res.cpu().numpy(), cnt.cpu().numpy().tolist()


def raw(be):
    """every byte the reports can see: state rows, summary, bodies, contacts"""
    p, b, a = be.state_tensors()
    return [x.cpu().numpy().tobytes() for x in (p, b, a, be.summary(), *be.bodies(), *be.contacts())]


def check_against_ref(be, case, flags=None, before=None, what=""):
    """add_particles on `be` == the restatement on what load_scene returned before; returns (after, result, counts)"""
    flags = case["flags"] if flags is None else flags
    before = load_all(be, case["bufs"]) if before is None else before
    want = cases.expected(case, flags, loaded=before)
    res, cnt = add(be, case["rows"], flags)
    for i, (edited, r, c) in enumerate(want):
        print(what, "scene", i, "result", res[i].tolist(), "want", r.tolist(), "counts", cnt[i], c)
    for i, (edited, r, c) in enumerate(want):
        assert res[i].tolist() == r.tolist() and cnt[i] == c, (what, i)
    after = [None if b is None else be.load_scene(i, b.copy()) for i, b in enumerate(before)]
    for i, (edited, _, _) in enumerate(want):
        if edited is not None:
            assert_same(after[i], edited, "%s: scene %d after the add == the restatement's edit" % (what, i))
    return after, res, cnt


def oracle_frames(oracle, buf, frames, mode):
    r = oracle.OracleEngine(1000.0, 10.0, 64, buf.layout, mode, threads=4)
    r.write_buffers(buf)
    for _ in range(frames):
        r.frame()
    return r.load_buffers(buf.copy())


@pytest.mark.parametrize("mode", [pytest.param(OFF, id="off"), pytest.param(GRID, id="default")])
def test_restatement_then_oracle(sb, oracle, mode):
    """the edit against the restatement: eight default scenes, each with its own rows; then two frames against the oracle from the
    edited scenes, contacts on and off: one spawned particle hits the left wall, one falls onto the body"""
    case = cases.default_case(sb)
    be = batch(sb, case, mode)
    after, res, cnt = check_against_ref(be, case, what="default")
    assert sum(c[0] for c in cnt) == 24
    be.frame(2)
    got = load_all(be, after)
    for i, b in enumerate(after):
        assert_same(got[i], oracle_frames(oracle, b, 2, ALLPAIRS if mode else OFF), "scene %d: two frames after the add == oracle" % i)
        assert got[i].particles[119, 2] > 0.0, "the wall turned the first particle round"
    assert be.info("add_particles_kernel_vgprs") > 0 and be.info("add_particles_kernel_scratch_bytes") == 0
    be.destroy()


def test_equals_the_host_route(sb):
    """add_particles == write_scene of the host-edited scene: load_scene, the reports, and the state two frames later"""
    case = cases.default_case(sb)
    a, b = batch(sb, case, GRID), batch(sb, case, GRID)
    want = cases.expected(case)
    add(a, case["rows"])
    upload_each(b, [w[0] for w in want])
    for i, (ga, gb) in enumerate(zip(load_all(a, case["bufs"]), load_all(b, case["bufs"]))):
        assert_same(ga, gb, "scene %d: device route == host route" % i)
    assert raw(a) == raw(b)
    for x in (a, b):
        x.frame(2)
    assert raw(a) == raw(b)
    for i, (ga, gb) in enumerate(zip(load_all(a, case["bufs"]), load_all(b, case["bufs"]))):
        assert_same(ga, gb, "scene %d: device route == host route after two frames" % i)
    a.destroy()
    b.destroy()


def test_row_codes(sb):
    """every code in one scene under SKIP_TOUCHING -- exactly 2r away is added, one ulp closer and a coincident row are BLOCKED,
    the blocked rule's three cases -- and the same rows without the flag"""
    case = cases.codes_case(sb)
    for flags, codes, counts in ((ref.SKIP_TOUCHING, [119, B, B, I, I, I, I, E, 120, B, B, B, 121, 122, 123], [5, 4, 5, 0]),
                                 (0, [119, 120, 121, I, I, I, I, E, 122, 123, 124, 125, 126, 127, FULL], [9, 4, 0, 1])):
        be = batch(sb, case)
        _, res, cnt = check_against_ref(be, case, flags, what="codes, flags %d" % flags)
        assert res[0].tolist() == codes and cnt == [counts]
        be.destroy()


def test_room(sb):
    """P = cap - 3 with five rows: three added, two FULL; a full scene; a scene never uploaded (all INVALID, its blobs untouched)"""
    case = cases.room_case(sb)
    be = batch(sb, case)
    before = raw(be)
    _, res, cnt = check_against_ref(be, case, what="room")
    assert res.tolist() == [[16, 17, 18, FULL, E, FULL], [FULL] * 4 + [E, FULL], [I] * 4 + [E, I]]
    assert cnt == [[3, 0, 0, 2], [0, 0, 0, 5], [0, 5, 0, 0]]
    plain = batch(sb, case)
    for x, y in zip(be.state_tensors(), plain.state_tensors()):
        assert x[1:].cpu().numpy().tobytes() == y[1:].cpu().numpy().tobytes(), "the full and the never-uploaded scene are untouched"
    assert raw(be) != before and be.summary().cpu().numpy()[:, 0].tolist() == [19.0, 19.0, 0.0]
    be.destroy()
    plain.destroy()


def test_sparse_mapping_takes_the_smallest_free_index(sb, oracle):
    case = cases.sparse_case(sb)
    be = batch(sb, case)
    after, res, cnt = check_against_ref(be, case, what="sparse")
    assert res[0].tolist() == [1, 4, 6] and after[0].mapping[16:19].tolist() == [1, 4, 6] and after[0].particle_count == 19
    be.frame()
    assert_same(be.load_scene(0, after[0].copy()), oracle_frames(oracle, after[0], 1, OFF), "the frame after == oracle")
    be.destroy()


def test_reset_removes_the_particle_and_its_weld(sb):
    """reset removes the particle and the weld onto it, summary()'s counts return; three spawn - reset episodes in a scene with one
    free slot all succeed; checkpoint then reset keeps it"""
    case = cases.one_free_case(sb)
    be = batch(sb, case)
    upload = raw(be)
    loaded = load_all(be, case["bufs"])
    for episode in range(3):
        res, cnt = add(be, case["rows"])
        assert res.tolist() == [[16]] and cnt == [[1, 0, 0, 0]], episode
        weld = beam_ref.pack([(16, 3, 0.0) + cases.MAT])[None]
        wres, wcnt = be.add_beams(dev(weld), length_current=True)
        assert wres.cpu().numpy().tolist() == [[42]] and wcnt.cpu().numpy().tolist() == [[1, 0, 0, 0]]
        assert be.summary().cpu().numpy()[0, :2].tolist() == [17.0, 43.0] and be.bodies()[1].cpu().numpy()[0, 0] == 1
        be.frame()
        be.reset()
        s = be.summary().cpu().numpy()[0]
        assert s[:4].tolist() == [16.0, 42.0, 1.0, 0.0], "16 particles and 42 beams again; the weld's index reads removed"
        back = raw(be)
        assert back[0] == upload[0] and back[2] == upload[2] and back[4:] == upload[4:], "particles, alive, bodies and contacts as uploaded"
        got = be.load_scene(0, loaded[0].copy())
        want, held = ref.reset_ref(ref.add_ref(loaded[0], case["rows"][0])[0], loaded[0], 16)
        assert got.metadata.tobytes() == want.metadata.tobytes() and got.mapping.tobytes() == want.mapping.tobytes()
        assert got.particles.tobytes() == want.particles.tobytes() and not held[16]
    full = add(be, np.concatenate([case["rows"], case["rows"]], axis=1))
    assert full[0].tolist() == [[16, FULL]]
    be.checkpoint()
    be.frame(2)
    be.reset()
    assert be.summary().cpu().numpy()[0, 0] == 17.0, "checkpoint then reset keeps it"
    assert add(be, case["rows"])[0].tolist() == [[FULL]]
    be.destroy()


def test_fork_and_masks(sb):
    """fork copies a spawned particle, with and without as_reset; a masked reset leaves unmasked scenes' spawns alone"""
    import torch
    case = cases.sparse_case(sb)
    buf, rows = case["bufs"][0], case["rows"][0]
    four = dict(case, bufs=[buf] * 4, rows=np.stack([rows, np.full_like(rows, -1), np.full_like(rows, -1), rows]))
    be = batch(sb, four)
    res, cnt = add(be, four["rows"])
    assert cnt == [[3, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [3, 0, 0, 0]]
    spawned = [x.cpu().numpy()[0].tobytes() for x in be.state_tensors()]
    keep = -1
    be.fork(torch.tensor([keep, 0, keep, keep], dtype=torch.int32, device="cuda"))
    be.fork(torch.tensor([keep, keep, 0, keep], dtype=torch.int32, device="cuda"), as_reset=True)
    for s in (1, 2):
        assert [x.cpu().numpy()[s].tobytes() for x in be.state_tensors()] == spawned
    assert be.summary().cpu().numpy()[:, 0].tolist() == [19.0] * 4
    be.frame()
    be.reset(torch.tensor([0, 1, 1, 1], dtype=torch.uint8, device="cuda"))
    # scene 0: unmasked, keeps its spawn (and has moved); 1: the source's reset state, the upload; 2: the forked state; 3: the upload
    assert be.summary().cpu().numpy()[:, 0].tolist() == [19.0, 16.0, 19.0, 16.0]
    assert [x.cpu().numpy()[2].tobytes() for x in be.state_tensors()] == spawned, "the forked state is the reset state"
    plain = batch(sb, four)
    for x, y in zip(be.state_tensors(), plain.state_tensors()):
        assert x[[1, 3]].cpu().numpy().tobytes() == y[[1, 3]].cpu().numpy().tobytes()
    # the indices are free again in 1 and 3, taken in 0 and 2
    res, cnt = add(be, np.stack([rows] * 4))
    assert res.tolist() == [[9, 11, 14], [1, 4, 6], [9, 11, 14], [1, 4, 6]]
    be.destroy()
    plain.destroy()


def test_dry_run_and_what_later_calls_see(sb):
    """a dry run leaves the batch bit for bit as it was; write_particles_device, state_tensors, summary, bodies, contacts, graph and
    render see the new particle; render against render_ref for one scene"""
    import render_ref
    import torch
    case = cases.codes_case(sb)
    be = batch(sb, case, GRID)
    be.frame()
    before, scenes = raw(be), load_all(be, case["bufs"])
    dres, dcnt = add(be, case["rows"], ref.SKIP_TOUCHING, dry=True)
    assert raw(be) == before
    for got, was in zip(load_all(be, case["bufs"]), scenes):
        assert_same(got, was, "a dry run")
    after, res, cnt = check_against_ref(be, case, before=scenes, what="after a frame")
    assert res.tolist() == dres.tolist() and cnt == dcnt and raw(be) != before
    new = [int(d) for d in res[0] if d >= 0]
    p, _, _ = be.state_tensors()
    assert not torch.isnan(p[0, new, :2]).any() and be.summary().cpu().numpy()[0, 0] == 119.0 + len(new)
    labels, counts = (x.cpu().numpy() for x in be.bodies())
    assert labels[0, new].tolist() == new, "each new particle is a body of its own"
    touch, ccounts = (x.cpu().numpy() for x in be.contacts())
    wt, _, wc = batch_contacts_ref.contacts_of(after, 128)
    assert np.array_equal(touch, wt) and np.array_equal(ccounts, wc)
    g = be.graph(ends=True, adjacency=True)
    assert g.row_ptr.cpu().numpy()[0, new[0]] == g.row_ptr.cpu().numpy()[0, new[0] + 1], "no beam on a new particle"
    moved = p.clone()
    moved[0, new[0], :2] = torch.tensor([700.0, 700.0], device="cuda")
    be.write_particles_device(moved)
    assert be.state_tensors()[0][0, new[0], :2].cpu().numpy().tolist() == [700.0, 700.0]
    now = be.load_scene(0, after[0].copy())
    pic = be.render(resolution=64).cpu().numpy()[0]
    assert np.array_equal(pic, render_ref.render_ref(now, 64, 1000.0, 10.0)), "the picture shows the new particles"
    be.destroy()


def test_spawn_a_body(sb, oracle):
    """add_particles -> body_beam_rows -> add_beams spawns a triangle: bodies() counts one more body, two frames match the oracle"""
    import torch
    buf = sb.scenes.default_buffers(1, *cases.DEFAULT_CAP)
    case = dict(layout=1, cap=cases.DEFAULT_CAP, bufs=[buf, buf], rows=cases.triangle_rows(2), flags=0)
    be = batch(sb, case, GRID)
    n_bodies = be.bodies()[1].cpu().numpy()[:, 0].copy()
    pos = dev(case["rows"][:, :, 1:3].copy(), np.float32)
    vel = dev(case["rows"][:, :, 3:5].copy(), np.float32)
    rows = sb.batch.new_particle_rows(pos, vel)
    assert rows.is_cuda and rows.cpu().numpy().tobytes() == case["rows"].tobytes()
    res, cnt = be.add_particles(rows, skip_touching=True)
    assert res.cpu().numpy().tolist() == [[119, 120, 121]] * 2 and cnt.cpu().numpy().tolist() == [[3, 0, 0, 0]] * 2
    beams = sb.batch.body_beam_rows(res, cases.TRIANGLE_EDGES, 30.0, *cases.MAT)
    want = np.stack([beam_ref.pack([(119 + a, 119 + b, 30.0) + cases.MAT for a, b in cases.TRIANGLE_EDGES])] * 2)
    assert beams.is_cuda and beams.cpu().numpy().tobytes() == want.tobytes()
    wres, wcnt = be.add_beams(beams)
    assert wres.cpu().numpy().tolist() == [[299, 300, 301]] * 2 and wcnt.cpu().numpy().tolist() == [[3, 0, 0, 0]] * 2
    assert (be.bodies()[1].cpu().numpy()[:, 0] == n_bodies + 1).all()
    # a row is empty wherever an endpoint's result is negative
    partial = torch.tensor([[119, ref.FULL, 121]], dtype=torch.int32, device="cuda")
    pr = sb.batch.body_beam_rows(partial, cases.TRIANGLE_EDGES, 30.0, *cases.MAT).cpu().numpy()
    assert pr[0, :, 0].tolist() == [-1, -1, 121] and pr[0, :, 1].tolist() == [-1, -1, 119]
    # edges already on the device are not read back: an index outside the call's rows gives an empty row, never a wrapped one
    on_dev = torch.tensor([[0, 1], [2, -1], [3, 0]], dtype=torch.int64, device="cuda")
    dr = sb.batch.body_beam_rows(res, on_dev, 30.0, *cases.MAT).cpu().numpy()
    assert dr[:, :, 0].tolist() == [[119, -1, -1]] * 2 and dr[:, 0, 1].tolist() == [120, 120]
    # new_particle_rows with an acceleration and a mask of rows that count
    acc = torch.tensor([0.0, -0.25], device="cuda")
    masked = sb.batch.new_particle_rows(pos, vel, acc, valid=torch.tensor([True, False, True], device="cuda")).cpu().numpy()
    want = case["rows"].copy()
    want[:, :, 5:7] = np.asarray([0.0, -0.25], "f4").view(np.int32)
    want[:, 1, 0] = -1
    assert masked.tobytes() == want.tobytes()
    after = load_all(be, case["bufs"])
    be.frame(2)
    for i, got in enumerate(load_all(be, after)):
        assert_same(got, oracle_frames(oracle, after[i], 2, ALLPAIRS), "scene %d: two frames after spawning a body == oracle" % i)
    be.destroy()
