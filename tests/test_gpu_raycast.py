"""Engine.raycast (sb_raycast_device / sb_raycast) on the GPU, every comparison bit for bit (np.array_equal) against
tests/raycast_ref.py -- brute force with the wide key -- on what load_buffers returns: the twelve scenes of the batch's case set on an
Engine, equal to BatchEngine.raycast too, without labels, with bodies()' labels and with stale ones; a 32 x 32 lattice at
cells_per_side 1, 2, 3 and the default rule; leftovers; after a cut, the delete pass and a plan-keeping re-upload; the call only reads;
each output alone; the host copy; every error code in order (UNSUPPORTED through ghost zones); no scratch.  Outputs are pre-filled with a pattern."""
import ctypes

import numpy as np
import pytest

import batch_raycast_cases as cases
import batch_raycast_ref as bref
import bodies_cases as bc
import raycast_ref as ref
import report_harness as rh
from batch_harness import make_batch, upload_each
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

OFF, GRID = 0, 2
F = np.float32
INF = ref.INF
BOUNDS = 4000.0


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def cast(eng, rows, labels=None, **kw):
    """the three outputs as numpy (t as float32), written into tensors the test filled with a pattern first"""
    import torch
    n = rows.shape[0]
    t = torch.full((n,), -7.25, dtype=torch.float32, device="cuda")
    hit = torch.full((n, 3), -1515870811, dtype=torch.int32, device="cuda")
    counts = torch.full((8,), -77, dtype=torch.int64, device="cuda")
    got = eng.raycast(dev(rows), labels=labels if labels is None or labels is True else dev(labels), t=t, hit=hit, counts=counts, **kw)
    assert got.t is t and got.hit is hit and got.counts is counts
    return ref.RayCast(*(x.cpu().numpy() for x in got))


def check(eng, buf, rows, labels=None, what="", bounds=cases.BOUNDS, radius=cases.RADIUS, **kw):
    """raycast() == the restatement on what load_buffers returns now; returns (the scene as read back, the result)"""
    now = eng.load_buffers(buf.copy())
    want = ref.raycast_ref(now, rows, bounds, radius, labels, cells_per_side=kw.get("cells_per_side", 0))
    got = cast(eng, rows, labels, **kw)
    print(what, "counts", got.counts.tolist(), "want", want.counts.tolist())
    assert ref.same(got, want) == [], (what, ref.same(got, want))
    return now, got


@pytest.mark.parametrize("mode", [OFF, GRID])
def test_case_set_equals_reference_and_batch(sb, mode):
    """the twelve scenes on an Engine each: the reference, BatchEngine.raycast on the same scenes, the stated answers; without
    labels, with bodies()' labels, with stale arbitrary labels"""
    cs = cases.case_set(sb)
    bufs, rows, labels = cases.stacked(cs)
    be = make_batch(sb, dict(layout=cases.LAYOUT, cap=cases.CAP, bufs=bufs, mode=mode), mode=mode)
    upload_each(be, bufs)
    rng = np.random.default_rng(9)
    stale = rng.integers(-2 ** 31, 2 ** 31, labels.shape, dtype=np.int64).astype(np.int32)
    stale[:, ::3] = rng.integers(0, 5, stale[:, ::3].shape)
    skipping = rows.copy()
    skipping[:, ::2, 6] = rng.integers(0, 5, skipping[:, ::2, 6].shape)
    batch = {}
    for name, r, lab in (("plain", rows, None), ("labelled", rows, labels), ("stale", skipping, stale)):
        got = be.raycast(dev(r), labels=None if lab is None else dev(lab))
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
            assert np.array_equal(got.t.view(np.uint32), batch[name][0][i].view(np.uint32)) and np.array_equal(got.hit, batch[name][1][i]), (c["name"], name, "the batch's rows")
            assert got.counts[:4].tolist() == batch[name][2][i].tolist()
            for j, (t, kind, index) in (c[key].items() if key else ()):
                assert (got.t[j].view(np.uint32), got.hit[j, 0], got.hit[j, 1]) == (F(t).view(np.uint32), kind, index), (c["name"], j)
            kinds |= set(got.hit[:, 0].tolist())
        assert ref.same(cast(eng, rows[i], True), cast(eng, rows[i], labels[i])) == [], "labels=True == bodies()' labels"
        eng.destroy()
    assert kinds == {-2, -1, 0, 1, 2, 3}


def lattice(sb, w=32, h=32):
    return sb.scenes.lattice_buffers(w, h, d=30.0, origin=(100.0, 100.0), strain_limit=0.5, layout=2, slack=5)


def lattice_rows(buf, seed=5, n=160):
    """drawn rays over the lattice of spacing 30 at (100, 100): along cell borders, diagonal, short and endless, from outside the box,
    from beyond the gate, a zero direction, every mask"""
    rng = np.random.default_rng(seed)
    rows = []
    for j in range(n):
        mask = 1 + j % 7
        tmax = float(rng.uniform(5.0, 200.0)) if j % 3 == 0 else INF
        kind = j % 8
        if kind == 0:     # axis-parallel, along a border of the cells of 125 (cells_per_side 32) and of 2000 (2)
            rows.append((mask, -50.0, 125.0 * (j % 9), 1.0, 0.0, tmax))
        elif kind == 1:
            rows.append((mask, 2000.0, 4100.0, 0.0, -1.0, tmax))
        elif kind == 2:   # diagonal through cell corners and lattice nodes
            rows.append((mask, 125.0 * (j % 5), 125.0 * (j % 5), 1.0, 1.0, tmax))
        elif kind == 3:   # from outside the box
            rows.append((mask, *rng.uniform(-3000.0, 7000.0, 2), *rng.normal(size=2), tmax))
        elif kind == 4:   # beyond the gate: the sweep answers it
            rows.append((mask, -4000.5 - 100.0 * (j % 3), float(rng.uniform(100.0, 1000.0)), 1.0, float(rng.uniform(-0.05, 0.05)), INF))
        else:             # inside the lattice, aimed anywhere, unit and long directions
            d = rng.normal(size=2) * (100.0 if j % 5 == 0 else 1.0)
            rows.append((mask, *rng.uniform(80.0, 1100.0, 2), *d, tmax / max(float(np.hypot(*d)), 1e-3) if np.isfinite(tmax) else INF))
    rows += [(7, 500.0, 500.0, 0.0, 0.0, 5.0), (0, 0, 0, 0, 0, 0), (8, 0, 0, 1, 0, 1)]   # a zero direction (swept), an empty and an invalid row
    return bref.pack(rows)


def test_lattice_at_every_cells_per_side(sb):
    buf = lattice(sb)
    eng = rh.engine(sb, buf, BOUNDS, collision_mode=OFF)
    rows = lattice_rows(buf)
    assert eng.info("raycast_cells_per_side") == ref.grid(buf.particle_count, BOUNDS, 10.0)[0] == 22
    out = {}
    for cps in (1, 2, 3, 0):
        _, out[cps] = check(eng, buf, rows, None, "32 x 32, cells_per_side %d" % cps, bounds=BOUNDS, cells_per_side=cps)
        assert ref.same(out[cps][:2] + (None,), out[1][:2] + (None,)) == [], "t and hit do not depend on the cells"
    c = out[0].counts
    assert c[4] >= 160 // 8 + 1 and c[5] == 0 and c[6] == 0 and c[1] > 20 and c[2] > 20 and c[3] > 5, c.tolist()
    assert out[1].counts[6] == 0 and out[3].counts.tolist() == c.tolist()
    labels, _ = eng.bodies()
    skip = rows.copy()
    skip[::2, 6] = 0     # the lattice is body 0: every second row sees past all of it
    _, got = check(eng, buf, skip, labels.cpu().numpy(), "32 x 32, its own body skipped", bounds=BOUNDS)
    assert not (got.hit[::2, 0] == 1).any() and not (got.hit[::2, 0] == 2).any() and (got.hit[1::2, 2][got.hit[1::2, 0] > 0][got.hit[1::2, 0][got.hit[1::2, 0] > 0] < 3] == 0).all()
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
    rows = bref.pack([(7, 3000.0, 3000.0, -1.0, -1.0, INF), (2, 3500.0, 3500.0, -1.0, -1.0, INF), (7, 10.0, 300.0, 1.0, 0.0, INF),
                      (1, 3000.0, -500.0, 0.0, 1.0, INF), (7, 130.0, 50.0, 0.0, 1.0, INF)] + [tuple(r) for r in lattice_rows(buf, 8, 40).view(F)[:, :6].tolist()])
    rows[5:, 0] = lattice_rows(buf, 8, 40)[:, 0]
    _, got = check(eng, buf, rows, None, "a beam across the box", bounds=BOUNDS)
    assert got.counts[5] == 0 and got.counts[6] == 1 and got.hit[1].tolist()[:2] == [2, B], got.hit[:2].tolist()
    st = eng.state_tensors()["particles"]
    st[0, 0] = float("nan")
    st[5, :2] = torch.tensor([3000.0, -300.0], device="cuda")
    eng.write_particles_device(st)
    now, got = check(eng, buf, rows, None, "NaN and outside", bounds=BOUNDS)
    assert got.counts[5] == 2 and got.counts[6] >= 1 + 3 + 3, got.counts.tolist()
    assert got.hit[3].tolist()[:2] == [1, 5] and got.t[3] == 190.0, "the particle outside the box is met, exactly"
    eng.destroy()


@pytest.mark.parametrize("mode", [OFF, GRID])
def test_cut_delete_pass_and_reupload(sb, mode):
    buf = lattice(sb, 20, 20)
    eng = rh.engine(sb, buf, BOUNDS, collision_mode=mode)
    x_cut = 100.0 + 30.0 * 9.5
    rows = bref.pack([(2, x_cut, 100.0 + 30.0 * k, 0.0, 1.0, INF) for k in range(6)] + [(2, 90.0, 100.0 + 30.0 * k + 7.0, 1.0, 0.0, INF) for k in range(6)])
    _, before = check(eng, buf, rows, None, "uploaded", bounds=BOUNDS)
    hit, c = eng.cut(sb.cut_shapes(segments=[(x_cut, 0.0, x_cut, 2000.0)]), hit=True)
    hit = np.asarray(hit.cpu() if hasattr(hit, "cpu") else hit).astype(bool)
    _, pending = check(eng, buf, rows, None, "cut pending", bounds=BOUNDS)
    assert ref.same(pending, before) == [] and hit[pending.hit[:6, 1]].all(), "a pending flag is still met"
    eng.delete_pass()
    now, after = check(eng, buf, rows, None, "after the delete pass", bounds=BOUNDS)
    assert now.beam_count == buf.beam_count - hit.sum() and not hit[after.hit[:, 1][after.hit[:, 0] == 2]].any(), "a removed beam is no longer met"
    assert (after.hit[:6, 0] == 0).all() and (after.hit[6:, 0] == 2).all()
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
    assert (got.hit[:6, 0] == 0).all() and eng.info("raycast_table_build_us") > 0
    eng.destroy()


def test_read_only_outputs_host_and_errors(sb):
    import torch
    buf = lattice(sb, 12, 12)
    rows = lattice_rows(buf, 3, 64)
    out = {}
    for k in ("plain", "read"):
        eng = rh.engine(sb, buf, BOUNDS, collision_mode=GRID)
        eng.frame()
        if k == "read":
            cast(eng, rows)
            cast(eng, rows, True, cells_per_side=3)
            eng.raycast_host(rows)
        eng.frame()
        out[k] = eng.load_buffers(buf.copy())
        if k == "plain":
            eng.destroy()
    assert_same(out["read"], out["plain"], "frame, raycast, frame == frame, frame")
    # each output alone; the defaults; the host copy; no rays
    lab = eng.bodies()[0]
    full = cast(eng, rows, lab.cpu().numpy())
    r = dev(rows)
    for i, name in enumerate(ref.RayCast._fields):
        want = [False] * 3
        want[i] = True
        got = eng.raycast(r, labels=lab, t=want[0], hit=want[1], counts=want[2])
        assert [x is not None for x in got] == want and np.array_equal(got[i].cpu().numpy().view(np.int32 if i < 2 else np.int64), full[i].view(np.int32 if i < 2 else np.int64)), name
    assert ref.same(ref.RayCast(*(x.cpu().numpy() for x in eng.raycast(r, labels=lab))), full) == []
    assert ref.same(eng.raycast_host(rows, lab.cpu().numpy()), full) == [], "sb_raycast == sb_raycast_device"
    assert ref.same(eng.raycast_host(rows.view(F), cells_per_side=2), cast(eng, rows)) == []
    z = eng.raycast(r[:0].contiguous())
    assert z.t.shape == (0,) and z.hit.shape == (0, 3) and not z.counts.cpu().numpy().any()
    packed = sb.engine.ray_rows(torch.tensor(rows[:, 1:3].copy().view(F)).cuda(), torch.tensor(rows[:, 3:5].copy().view(F)).cuda(),
                                torch.tensor(rows[:, 5].copy().view(F)).cuda(), mask=dev(rows[:, 0].copy()), skip_label=dev(rows[:, 6].copy()))
    assert packed.shape == (len(rows), 8) and np.array_equal(packed.cpu().numpy().view(np.uint32)[:, :7], rows[:, :7]), "ray_rows packs [n] rows"
    # errors, in order: INVALID before STATE before UNSUPPORTED; nothing is enqueued
    lib = sb.engine.load_library()
    vp = ctypes.c_void_p
    outs = [torch.full((k,), 77, dtype=dt, device="cuda") for k, dt in ((64, torch.int32), (64 * 3, torch.int32), (8, torch.int64), (eng.max_particles, torch.int32))]
    t, h, c, lp = (x.data_ptr() for x in outs)
    rp = r.data_ptr()
    torch.cuda.synchronize()

    def opts(flags=0, cps=0, size=None, reserved=0):
        o = sb.engine.SbRaycastOptions()
        o.struct_size = ctypes.sizeof(o) if size is None else size
        o.flags, o.cells_per_side = flags, cps
        o.reserved[2] = reserved
        return o

    fresh = sb.Engine(bounds_size=BOUNDS, layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=OFF)
    for e in (eng, fresh):   # (an INVALID argument is INVALID before an upload too)
        for hnd, o, rays, n, args in ((None, opts(), rp, 64, (lp, t, h, c)), (e._h, opts(flags=1), rp, 64, (lp, t, h, c)), (e._h, opts(size=8), rp, 64, (lp, t, h, c)),
                                      (e._h, opts(reserved=1), rp, 64, (lp, t, h, c)), (e._h, opts(), None, 64, (lp, t, h, c)), (e._h, opts(), rp, 64, (lp, None, None, None)),
                                      (e._h, opts(), rp, 0, (None, None, None, None)), (e._h, opts(), rp + 2, 64, (lp, t, h, c)), (e._h, opts(), rp, 64, (lp + 1, t, h, c)),
                                      (e._h, opts(), rp, 64, (lp, t + 2, h, c)), (e._h, opts(), rp, 64, (lp, t, h + 3, c)), (e._h, opts(), rp, 64, (lp, t, h, c + 4)),
                                      (e._h, opts(), rp, 2 ** 24 + 1, (lp, t, h, c)), (e._h, opts(cps=8193), rp, 64, (lp, t, h, c))):
            assert lib.sb_raycast_device(hnd, ctypes.byref(o), vp(rays), n, *[vp(p) for p in args]) == 1, (o.flags, n, args)
    assert lib.sb_raycast_device(fresh._h, None, vp(rp), 64, None, vp(t), None, None) == 5, "SB_ERR_STATE before an upload"
    assert lib.sb_raycast_device(fresh._h, None, None, 0, None, vp(t), None, None) == 5
    fresh.destroy()
    assert lib.sb_raycast_device(eng._h, None, None, 0, None, vp(t), vp(h), vp(c)) == 0, "no rays: nothing done"
    # UNSUPPORTED: an engine with ghost zones (a capacity above 2^30 is no test of a few seconds: 4 GiB of tables); INVALID still first
    small = sb.scenes.default_buffers(2, 256, 512)
    ghost = sb.Engine(layout=2, max_particles=256, max_beams=512, collision_mode=OFF, path=2)
    ghost.write_buffers(small)
    ghost.halo_configure([0, 1], [2, 3])
    assert lib.sb_raycast_device(ghost._h, None, vp(rp), 4, None, vp(t), vp(h), vp(c)) == 6, "SB_ERR_UNSUPPORTED with ghost zones"
    assert lib.sb_raycast_device(ghost._h, None, vp(rp), 4, None, None, None, None) == 1, "INVALID before UNSUPPORTED"
    with pytest.raises(sb.EngineError) as err:
        ghost.raycast_host(rows[:4])
    assert err.value.status == 6
    ghost.destroy()
    eng.sync()
    assert all((x.cpu().numpy() == 77).all() for x in outs), "no output was touched"
    for bad in (r[:, :7].contiguous(), r.to(torch.int64), r[None]):
        with pytest.raises(ValueError):
            eng.raycast(bad)
    with pytest.raises(ValueError):
        eng.raycast(r, t=False, hit=False, counts=False)
    assert eng.info("raycast_kernel_scratch_bytes") == 0 and 0 < eng.info("raycast_kernel_vgprs") <= 128
    eng.destroy()
