"""Engine.nearest (sb_nearest_device / sb_nearest) on the GPU, every comparison bit for bit against tests/nearest_ref.py
-- brute force with the wide key, and the ring rules behind word 4 -- on what load_buffers returns: the twelve scenes of the batch's
case set on an Engine, equal to BatchEngine.nearest too, without labels, with bodies()' labels and with stale ones; a 32 x 32 lattice
at cells_per_side 1, 2, 3, 0 crossed with max_rings 1, 2, 0, with and without within; leftovers; after a cut, the delete pass and a
plan-keeping re-upload; the call only reads; each output alone; the host copy; every error code.  Outputs are pre-filled with a
pattern."""
import ctypes

import numpy as np
import pytest

import batch_nearest_cases as cases
import batch_nearest_ref as bref
import bodies_cases as bc
import nearest_ref as ref
import report_harness as rh
from batch_harness import make_batch, upload_each
from test_gpu_parity import assert_same
from test_gpu_raycast import BOUNDS, dev, lattice

pytestmark = pytest.mark.gpu

OFF, GRID = 0, 2
F = np.float32
INF = ref.INF


def ask(eng, rows, labels=None, within=True, **kw):
    """the five outputs as numpy, written into tensors the test filled with a pattern first (within=False: left out)"""
    import torch
    n = rows.shape[0]
    d = torch.full((n,), -7.25, dtype=torch.float32, device="cuda")
    hit = torch.full((n, 3), -1515870811, dtype=torch.int32, device="cuda")
    point = torch.full((n, 2), -3.5, dtype=torch.float32, device="cuda")
    inside = torch.full((n, 2), -99, dtype=torch.int32, device="cuda") if within else False
    counts = torch.full((8,), -77, dtype=torch.int64, device="cuda")
    got = eng.nearest(dev(rows), labels=labels if labels is None or labels is True else dev(labels), d=d, hit=hit, point=point, within=inside, counts=counts, **kw)
    assert got.d is d and got.hit is hit and got.point is point and got.counts is counts and (got.within is inside if within else got.within is None)
    return ref.Nearest(*(None if x is None else x.cpu().numpy() for x in got))


def check(eng, buf, rows, labels=None, what="", bounds=cases.BOUNDS, within=True, **kw):
    """nearest() == the restatement on what load_buffers returns now; returns (the scene as read back, the result)"""
    now = eng.load_buffers(buf.copy())
    want = ref.nearest_ref(now, rows, bounds, 10.0, labels, cells_per_side=kw.get("cells_per_side", 0), max_rings=kw.get("max_rings", 0), within=within)
    got = ask(eng, rows, labels, within=within, **kw)
    print(what, "counts", got.counts.tolist(), "want", want.counts.tolist())
    assert ref.same(got, want) == [], (what, ref.same(got, want))
    return now, got


@pytest.mark.parametrize("mode", [OFF, GRID])
def test_case_set_equals_reference_and_batch(sb, mode):
    cs = cases.case_set(sb)
    bufs, rows, labels = cases.stacked(cs)
    be = make_batch(sb, dict(layout=cases.LAYOUT, cap=cases.CAP, bufs=bufs, mode=mode), mode=mode)
    upload_each(be, bufs)
    rng = np.random.default_rng(9)
    stale = rng.integers(-2 ** 31, 2 ** 31, labels.shape, dtype=np.int64).astype(np.int32)
    stale[:, ::3] = rng.integers(0, 5, stale[:, ::3].shape)
    skipping = rows.copy()
    skipping[:, ::2, 4] = rng.integers(0, 5, skipping[:, ::2, 4].shape)
    batch = {}
    for name, r, lab in (("plain", rows, None), ("labelled", rows, labels), ("stale", skipping, stale)):
        got = be.nearest(dev(r), labels=None if lab is None else dev(lab), d=True, hit=True, point=True, within=True, counts=True)
        batch[name] = [x.cpu().numpy() for x in got]
    be.destroy()
    kinds = set()
    for i, c in enumerate(cs):
        if c["buf"] is None:   # never uploaded: an engine has no such state (SB_ERR_STATE, below)
            continue
        eng = rh.engine(sb, c["buf"], cases.BOUNDS, collision_mode=mode)
        own, _ = eng.bodies()
        assert np.array_equal(own.cpu().numpy(), c["labels"]), "the host's labels of the case set are bodies()'s"
        for name, r, lab, key in (("plain", rows[i], None, "expect"), ("labelled", rows[i], labels[i], "expect_labelled"), ("stale", skipping[i], stale[i], None)):
            _, got = check(eng, c["buf"], r, lab, "%s, %s" % (c["name"], name))
            b = batch[name]
            assert ref.same(got, ref.Nearest(b[0][i], b[1][i], b[2][i], b[3][i], got.counts)) == [], (c["name"], name, "the batch's rows")
            assert got.counts[:4].tolist() == b[4][i].tolist()
            for j, (d, kind, index, qx, qy) in (c[key].items() if key else ()):
                assert (got.d[j].view(np.uint32), got.hit[j, 0], got.hit[j, 1]) == (F(d).view(np.uint32), kind, index), (c["name"], j)
                assert got.point[j].view(np.uint32).tolist() == np.asarray([qx, qy], F).view(np.uint32).tolist(), (c["name"], j)
            if key:
                inside = {**c["expect_within"], **(c["expect_within_labelled"] if name == "labelled" else {})}
                for j, pair in inside.items():
                    if name == "plain" and j in c["expect_within_labelled"]:
                        continue
                    if got.hit[j, 0] >= 0:
                        assert got.within[j].tolist() == list(pair), (c["name"], name, j)
            kinds |= set(got.hit[:, 0].tolist())
        assert ref.same(ask(eng, rows[i], True), ask(eng, rows[i], labels[i])) == [], "labels=True == bodies()' labels"
        eng.destroy()
    assert kinds == {-2, -1, 0, 1, 2, 3}


def lattice_points(seed=5, n=160):
    """drawn points over the 32 x 32 lattice of spacing 30 at (100, 100) in a box of 4000: on borders and corners of the cells of 125
    and 2000, on lattice nodes, mid-beam, outside the box, beyond the gate; rmax 0, small, a few cells, inf; every mask"""
    rng = np.random.default_rng(seed)
    rows = []
    reach = (0.0, 7.0, 31.0, 400.0, INF)
    for j in range(n):
        mask, rmax, kind = 1 + j % 7, reach[j % 5], j % 8
        if kind == 0:
            p = (125.0 * (j % 11), 125.0 * (j % 7))                      # a corner of the cells of 125
        elif kind == 1:
            p = (2000.0, float(rng.uniform(100.0, 1000.0))) if j % 16 == 1 else (float(rng.uniform(100.0, 1000.0)), 2000.0)
        elif kind == 2:
            p = (100.0 + 30.0 * (j % 32), 100.0 + 30.0 * (j % 29))       # a lattice node
        elif kind == 3:
            p = (115.0 + 30.0 * (j % 31), 100.0 + 30.0 * (j % 13))       # the middle of a beam
        elif kind == 4:
            p = tuple(rng.uniform(-3900.0, 7900.0, 2))                   # outside the box, inside the gate
        elif kind == 5:
            p = (-4000.5 - 100.0 * (j % 3), float(rng.uniform(100.0, 1000.0)))   # beyond the gate: the sweep answers it
        else:
            p = tuple(rng.uniform(80.0, 1100.0, 2))                      # anywhere in the lattice
        rows.append((mask, p[0], p[1], rmax))
    rows += [(7, 375.0, 500.0, 62.5), (0, 0, 0, 0), (8, 0, 0, 1)]        # on a border of 125, an empty and an invalid row
    return bref.pack(rows)


def test_lattice_at_every_cells_per_side_and_max_rings(sb):
    buf = lattice(sb)
    eng = rh.engine(sb, buf, BOUNDS, collision_mode=OFF)
    rows = lattice_points()
    assert eng.info("nearest_cells_per_side") == eng.info("raycast_cells_per_side") == 22 and eng.info("nearest_max_rings") == ref.DEFAULT_RINGS
    first, word4 = None, {}
    for cps in (1, 2, 3, 0):
        for rings in (1, 2, 0):
            for within in (True, False):
                _, got = check(eng, buf, rows, None, "32 x 32, cells_per_side %d max_rings %d within %s" % (cps, rings, within), bounds=BOUNDS, within=within,
                               cells_per_side=cps, max_rings=rings)
                first = first or got
                assert ref.same(got, first, skip=("counts",) if within else ("counts", "within")) == [] and got.counts[:4].tolist() == first.counts[:4].tolist()
                word4[cps, rings, within] = int(got.counts[4])
    c = first.counts
    assert c[5] == 0 and c[6] == 0 and c[1] > 10 and c[2] > 10 and c[3] > 5, c.tolist()
    assert word4[0, 1, True] > word4[0, 0, True] >= 160 // 8 and word4[0, 1, False] > word4[0, 0, False], word4
    labels, _ = eng.bodies()
    skip = rows.copy()
    skip[::2, 4] = 0     # the lattice is body 0: every second row sees past all of it
    _, got = check(eng, buf, skip, labels.cpu().numpy(), "32 x 32, its own body skipped", bounds=BOUNDS)
    assert not np.isin(got.hit[::2, 0], (1, 2)).any() and not got.within[::2].any()
    eng.destroy()


def test_leftovers(sb):
    """a beam across the whole box, a particle moved outside the box and one set to NaN on the device: words 5 and 6, exact answers"""
    import torch
    buf = lattice(sb, 16, 16)
    P, B, maxP = buf.particle_count, buf.beam_count, buf.max_particles
    buf.particles[P, :2], buf.particles[P + 1, :2] = (50.0, 3900.0), (3950.0, 60.0)
    buf.mapping[P], buf.mapping[P + 1] = P, P + 1
    buf.particle_count = P + 2
    rec = buf.beams[int(buf.mapping[maxP])].copy()
    rec["a"], rec["b"] = P, P + 1
    rec["length"] = rec["target_length"] = rec["last_length"] = np.hypot(3900.0, 3840.0)
    buf.beams[B] = rec
    buf.mapping[maxP + B] = B
    buf.beam_count = B + 1
    eng = rh.engine(sb, buf, BOUNDS, collision_mode=OFF)
    rows = np.concatenate([bref.pack([(2, 2010.0, 2000.0, 50.0), (5, 3000.0, -290.0, 20.0), (7, 3000.0, 3000.0, INF), (3, 300.0, 300.0, INF)]), lattice_points(8, 40)])
    _, got = check(eng, buf, rows, None, "a beam across the box", bounds=BOUNDS)
    assert got.counts[5] == 0 and got.counts[6] == 1 and got.hit[0].tolist()[:2] == [2, B], "the long beam wins a row"
    st = eng.state_tensors()["particles"]
    st[0, 0] = float("nan")
    st[5, :2] = torch.tensor([3000.0, -300.0], device="cuda")
    eng.write_particles_device(st)
    for within in (True, False):
        _, got = check(eng, buf, rows, None, "NaN and outside", bounds=BOUNDS, within=within)
        assert got.counts[5] == 2 and got.counts[6] >= 1 + 3 + 3, got.counts.tolist()
        assert got.hit[1].tolist()[:2] == [1, 5] and got.d[1] == 10.0 and got.point[1].tolist() == [3000.0, -300.0], "the particle outside the box wins, exactly"
    eng.destroy()


@pytest.mark.parametrize("mode", [OFF, GRID])
def test_cut_delete_pass_and_reupload(sb, mode):
    buf = lattice(sb, 20, 20)
    eng = rh.engine(sb, buf, BOUNDS, collision_mode=mode)
    x_cut = 100.0 + 30.0 * 9.5
    rows = bref.pack([(2, x_cut, 100.0 + 30.0 * k + 2.0, 5.0) for k in range(6)] + [(2, 90.0, 100.0 + 30.0 * k + 7.0, INF) for k in range(6)])
    _, before = check(eng, buf, rows, None, "uploaded", bounds=BOUNDS)
    hit, c = eng.cut(sb.cut_shapes(segments=[(x_cut, 0.0, x_cut, 2000.0)]), hit=True)
    hit = np.asarray(hit.cpu() if hasattr(hit, "cpu") else hit).astype(bool)
    _, pending = check(eng, buf, rows, None, "cut pending", bounds=BOUNDS)
    assert ref.same(pending, before) == [] and hit[pending.hit[:6, 1]].all() and (pending.within[:6, 1] >= 1).all(), "a pending beam still wins and counts"
    eng.delete_pass()
    now, after = check(eng, buf, rows, None, "after the delete pass", bounds=BOUNDS)
    assert now.beam_count == buf.beam_count - hit.sum() and not hit[after.hit[:, 1][after.hit[:, 0] == 2]].any(), "a removed beam no longer wins"
    assert (after.hit[:6, 0] == 0).all() and not after.within[:6].any() and (after.hit[6:, 0] == 2).all()
    eng.destroy()
    # a plan-keeping re-upload that removed beams (no delete pass runs)
    B = buf.beam_count
    rec = buf.beams[buf.mapping[buf.max_particles:buf.max_particles + B].astype(np.int64)]
    left = buf.particles[:, 0] < np.float32(x_cut)
    cut = bc.without(buf, left[rec["a"].astype(np.int64)] == left[rec["b"].astype(np.int64)])
    eng = rh.engine(sb, buf, BOUNDS, collision_mode=mode)
    check(eng, buf, rows, None, "whole again", bounds=BOUNDS)
    eng.write_buffers(cut)
    assert eng.info("uploads_edited") == 1
    _, got = check(eng, cut, rows, None, "re-uploaded without the crossing beams", bounds=BOUNDS)
    assert (got.hit[:6, 0] == 0).all() and not got.within[:6].any()
    eng.destroy()


def test_read_only_outputs_host_and_errors(sb):
    import torch
    buf = lattice(sb, 12, 12)
    rows = lattice_points(3, 64)
    out = {}
    for k in ("plain", "read"):
        eng = rh.engine(sb, buf, BOUNDS, collision_mode=GRID)
        eng.frame()
        if k == "read":
            ask(eng, rows)
            ask(eng, rows, True, cells_per_side=3, max_rings=1)
            eng.nearest_host(rows)
        eng.frame()
        out[k] = eng.load_buffers(buf.copy())
        st = {name: t.clone() for name, t in eng.state_tensors().items() if hasattr(t, "clone")}
        if k == "plain":
            plain_state = st
            eng.destroy()
    assert_same(out["read"], out["plain"], "frame, nearest, frame == frame, frame")
    assert all(torch.equal(st[name].view(torch.uint8), plain_state[name].view(torch.uint8)) for name in st), "and on state_tensors()"
    # each output alone; the defaults; the host copy; no points
    lab = eng.bodies()[0]
    full = ask(eng, rows, lab.cpu().numpy())
    r = dev(rows)
    for i, name in enumerate(ref.Nearest._fields):
        want = [False] * 5
        want[i] = True
        got = eng.nearest(r, labels=lab, d=want[0], hit=want[1], point=want[2], within=want[3], counts=want[4])
        assert [x is not None for x in got] == want, name
        words = ref.Nearest(*(None if x is None else x.cpu().numpy() for x in got))
        assert ref.same(words, full, skip=("counts",)) == [] and (i != 4 or words.counts[[0, 1, 2, 3, 5, 6, 7]].tolist() == full.counts[[0, 1, 2, 3, 5, 6, 7]].tolist()), name
    assert ref.same(ref.Nearest(*(x.cpu().numpy() for x in eng.nearest(r, labels=lab))), full) == []
    assert ref.same(eng.nearest_host(rows, lab.cpu().numpy()), full) == [], "sb_nearest == sb_nearest_device"
    assert ref.same(eng.nearest_host(rows.view(F), cells_per_side=2, max_rings=3), ask(eng, rows), skip=("counts",)) == []
    z = eng.nearest(r[:0].contiguous())
    assert z.d.shape == (0,) and z.hit.shape == (0, 3) and z.point.shape == (0, 2) and z.within.shape == (0, 2) and not z.counts.cpu().numpy().any()
    packed = sb.batch.point_rows(torch.tensor(rows[:, 1:3].copy().view(F)).cuda()[None], torch.tensor(rows[:, 3].copy().view(F)).cuda(),
                                 mask=dev(rows[:, 0].copy()), skip_label=dev(rows[:, 4].copy()))[0]
    assert np.array_equal(packed.cpu().numpy().view(np.uint32)[:, :5], rows[:, :5]), "batch.point_rows packs an engine's rows"
    # errors, in order: INVALID before STATE before UNSUPPORTED; nothing is enqueued
    lib = sb.engine.load_library()
    vp = ctypes.c_void_p
    outs = [torch.full((k,), 77, dtype=dt, device="cuda") for k, dt in ((64, torch.int32), (64 * 3, torch.int32), (64 * 2, torch.int32), (64 * 2, torch.int32),
                                                                      (8, torch.int64), (eng.max_particles, torch.int32))]
    d, h, q, w, c, lp = (x.data_ptr() for x in outs)
    rp = r.data_ptr()
    torch.cuda.synchronize()

    def opts(flags=0, cps=0, rings=0, size=None, reserved=0):
        o = sb.engine.SbNearestOptions()
        o.struct_size = ctypes.sizeof(o) if size is None else size
        o.flags, o.cells_per_side, o.max_rings = flags, cps, rings
        o.reserved[2] = reserved
        return o

    def call(hnd, o, points, n, args):
        return lib.sb_nearest_device(hnd, None if o is None else ctypes.byref(o), vp(points), n, *[vp(p) for p in args])

    ok = (lp, d, h, q, w, c)
    fresh = sb.Engine(bounds_size=BOUNDS, layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=OFF)
    for e in (eng, fresh):   # (an INVALID argument is INVALID before an upload too)
        for hnd, o, points, n, args in ((None, opts(), rp, 64, ok), (e._h, opts(flags=1), rp, 64, ok), (e._h, opts(size=8), rp, 64, ok),
                                        (e._h, opts(reserved=1), rp, 64, ok), (e._h, opts(), None, 64, ok), (e._h, opts(), rp, 64, (lp, None, None, None, None, None)),
                                        (e._h, opts(), rp, 0, (None,) * 6), (e._h, opts(), rp + 2, 64, ok), (e._h, opts(), rp, 64, (lp + 1, d, h, q, w, c)),
                                        (e._h, opts(), rp, 64, (lp, d + 2, h, q, w, c)), (e._h, opts(), rp, 64, (lp, d, h + 3, q, w, c)),
                                        (e._h, opts(), rp, 64, (lp, d, h, q + 1, w, c)), (e._h, opts(), rp, 64, (lp, d, h, q, w + 2, c)),
                                        (e._h, opts(), rp, 64, (lp, d, h, q, w, c + 4)), (e._h, opts(), rp, 2 ** 24 + 1, ok), (e._h, opts(cps=8193), rp, 64, ok),
                                        (e._h, opts(rings=8193), rp, 64, ok)):
            assert call(hnd, o, points, n, args) == 1, (o.flags, n, args)
    assert call(fresh._h, None, rp, 64, (None, d, None, None, None, None)) == 5, "SB_ERR_STATE before an upload"
    assert call(fresh._h, None, None, 0, (None, d, None, None, None, None)) == 5
    fresh.destroy()
    assert call(eng._h, None, None, 0, (None, d, h, q, w, c)) == 0, "no points: nothing done"
    # UNSUPPORTED: an engine with ghost zones (a capacity above 2^30 is no test of a few seconds); INVALID still first
    small = sb.scenes.default_buffers(2, 256, 512)
    ghost = sb.Engine(layout=2, max_particles=256, max_beams=512, collision_mode=OFF, path=2)
    ghost.write_buffers(small)
    ghost.halo_configure([0, 1], [2, 3])
    assert call(ghost._h, None, rp, 4, (None, d, h, q, w, c)) == 6, "SB_ERR_UNSUPPORTED with ghost zones"
    assert call(ghost._h, None, rp, 4, (None,) * 6) == 1, "INVALID before UNSUPPORTED"
    with pytest.raises(sb.EngineError) as err:
        ghost.nearest_host(rows[:4])
    assert err.value.status == 6
    ghost.destroy()
    eng.sync()
    assert all((x.cpu().numpy() == 77).all() for x in outs), "no output was touched"
    for bad in (r[:, :7].contiguous(), r.to(torch.int64), r[None]):
        with pytest.raises(ValueError):
            eng.nearest(bad)
    with pytest.raises(ValueError):
        eng.nearest(r, d=False, hit=False, point=False, within=False, counts=False)
    assert eng.info("nearest_kernel_scratch_bytes") == 0 and 0 < eng.info("nearest_kernel_vgprs") <= 128
    eng.destroy()
