"""The halo guard on the GPU (include/softbody.h sb_halo_guard, k_halo_guard): the device's verdict equals the numpy
restatement of the rule (tests/halo_guard_ref.py) refresh by refresh; Exchanger(guard=True) raises halo.RepartitionDue on
two clouds that fly into each other's slabs, while every frame before is bit-exact; it stays quiet, and changes no bit,
where the partition stays valid."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from halo_guard_ref import BAND, BEAM, SLAB, GuardModel, sound_reach  # noqa: E402

pytestmark = pytest.mark.gpu

CLOUD_DEPTH, CLOUD_REACH = 1, 130.0     # tests/test_halo_guard_cpu.py: R >= 3C at depth 1


def engine_for(sb, buf, mode=2, path=0, bounds=1000.0):
    e = sb.Engine(bounds_size=bounds, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams,
                  collision_mode=mode, path=path)
    e.write_buffers(buf)
    return e


def ranks(sb, made, mode, guard=True, motion=0.0, path=0, bounds=1000.0):
    import torch
    from halo_oracle import LocalBus
    dev = torch.device("cuda", 0)
    bus, exs, engs = LocalBus(), [], []
    for r, (lbuf, plan) in enumerate(made):
        eng = engine_for(sb, lbuf, mode, path, bounds)
        tr = bus.transport(r, lambda a, b: (torch.zeros(max(a, 1), device=dev), torch.zeros(max(b, 1), device=dev)),
                           lambda t: t.data_ptr())
        exs.append(sb.halo.Exchanger(eng, plan, tr, guard=guard, motion=motion))
        engs.append(eng)
    return bus, exs, engs


def sync_all(engs):
    import torch

    def sync():
        for e in engs:
            e.sync()
        torch.cuda.synchronize()
    return sync


def frame(bus, exs, engs):
    """frame_all (ranks in lock step) and then what Exchanger.frame() does at its end: the guard's verdict"""
    from halo_oracle import frame_all
    frame_all(exs, bus, lambda dst, src: dst.copy_(src), sync_all(engs))
    for ex in exs:
        ex.check_guard()


def gather(made, engs, n):
    got = None
    for (lbuf, plan), eng in zip(made, engs):
        out = eng.load_buffers(lbuf.copy())
        if got is None:
            got = np.zeros((n, 6), "<f4")
        got[plan.global_particle_id[plan.owned_particles]] = out.particles[plan.owned_particles]
    return got


def single_frames(sb, gbuf, frames, mode=2):
    ref = engine_for(sb, gbuf, mode)
    out = []
    for _ in range(frames):
        ref.frame()
        out.append(ref.load_buffers(gbuf.copy()).particles[:gbuf.particle_count].copy())
    ref.destroy()
    return out


def destroy(engs):
    for e in engs:
        e.destroy()


@pytest.mark.parametrize("scene", ["clouds", "default"])
def test_device_verdict_equals_the_model(sb, scene):
    """Refresh by refresh, on the read-back state of every rank: kinds, violation count, refreshes and first offending item
    of sb_halo_guard_status equal halo_guard_ref's.  Two clouds (checks A and B fire as they close in); the default scene
    with a motion allowance so large that H - 2Ds is shorter than its long beams (C)."""
    from halo_oracle import step_all
    from test_partition_cpu import two_clouds
    halo = sb.halo
    if scene == "clouds":
        gbuf, depth, motion, reach, refreshes = two_clouds(sb), CLOUD_DEPTH, 0.0, CLOUD_REACH, 450
    else:
        gbuf, depth, refreshes = sb.scenes.default_buffers(2, 256, 512), 2, 40
        H = halo.partition_scene(gbuf, 2, depth)[0][1].guard.hop
        motion = 0.2 * H
        reach = sound_reach(H, depth, motion)
    made = halo.partition_scene(gbuf, 2, depth, contact_reach=reach)
    bus, exs, engs = ranks(sb, made, 2, motion=motion)
    models = [GuardModel(plan, True, lbuf.particles, lbuf.beams, motion) for lbuf, plan in made]
    seen = 0
    for _ in range(refreshes):
        step_all(exs, bus, depth, lambda dst, src: dst.copy_(src), sync_all(engs))
        for (lbuf, plan), eng, m in zip(made, engs, models):
            m.refresh(eng.load_buffers(lbuf.copy()).particles, depth)
            st = eng.halo_guard_status()
            assert m.matches(st), (st, m.kinds, m.violations, m.refreshes, m.first)
            seen |= st.kinds
    destroy(engs)
    want = SLAB | BAND if scene == "clouds" else BEAM
    assert seen & want == want, seen


def test_two_clouds_raise_repartition_due(sb):
    """Without repartition: RepartitionDue at some frame f, and every frame before f is bit-exact with the single engine
    (the guard fires before the run goes wrong)."""
    from test_partition_cpu import two_clouds
    halo = sb.halo
    frames = 9
    gbuf = two_clouds(sb)
    wants = single_frames(sb, gbuf, frames)
    made = halo.partition_scene(gbuf, 2, CLOUD_DEPTH, contact_reach=CLOUD_REACH)
    bus, exs, engs = ranks(sb, made, 2)
    raised = None
    for f in range(frames):
        try:
            frame(bus, exs, engs)
        except halo.RepartitionDue as exc:
            raised = (f, exc)
            break
        assert np.array_equal(gather(made, engs, gbuf.particle_count).view("u4"), wants[f].view("u4")), "frame %d" % f
    assert raised is not None
    f, exc = raised
    plan = made[exc.rank][1]
    assert exc.kinds & (SLAB | BAND) and exc.kind_names and exc.violations > 0 and exc.refresh is not None
    assert not exc.is_beam and exc.global_id in set(plan.global_particle_id[plan.owned_particles].tolist())
    assert f < frames - 1
    for ex in exs:                                            # the non-raising view says the same
        st = ex.guard_status()
        assert st.refreshes == (f + 1) * 64
    destroy(engs)


def test_repartition_every_frame_never_raises(sb):
    """The guarded twin of test_gpu_halo's repartition test: re-partitioned after every frame, no raise, bit-exact."""
    from test_partition_cpu import two_clouds
    halo = sb.halo
    frames = 9
    gbuf = two_clouds(sb)
    want = single_frames(sb, gbuf, frames)[-1]
    made = halo.partition_scene(gbuf, 2, CLOUD_DEPTH, contact_reach=CLOUD_REACH)
    for f in range(frames):
        bus, exs, engs = ranks(sb, made, 2)
        frame(bus, exs, engs)
        states = [halo.owned_state(plan, eng.load_buffers(lbuf.copy())) for (lbuf, plan), eng in zip(made, engs)]
        destroy(engs)
        made = halo.repartition(gbuf, states, 2, CLOUD_DEPTH, CLOUD_REACH)
    P = gbuf.particle_count
    assert np.array_equal(gbuf.particles[:P].view("u4"), want.view("u4"))
    assert sum(p.ghost_p.size for _, plan in made for p in plan.peers) > 40


@pytest.mark.parametrize("scene,world,mode,path,depth", [
    ("default", 2, 1, 1, 1), ("default", 4, 2, 2, 1), ("pile", 2, 2, 2, 1), ("pile", 4, 1, 0, 2),
    ("pile", 2, 0, 2, 8), ("default", 4, 0, 2, 6)])
def test_no_false_alarms_and_no_changed_bits(sb, scene, world, mode, path, depth):
    """Quiet scenes partitioned with a sound reach, guard on for three frames: no raise, and every rank's state equals the
    guard-off run's bit for bit (collision modes 1 and 2, atomic / tiled / blocked paths; mode 0 runs the blocked kernel)."""
    halo = sb.halo
    if scene == "default":
        gbuf, bounds = sb.scenes.default_buffers(2, 256, 512), 1000.0
    else:
        gbuf, bounds = sb.scenes.blob_pile_buffers(9, 3, gap=19.6)
    H = halo.partition_scene(gbuf, world, depth)[0][1].guard.hop
    reach = sound_reach(H, depth) + H if mode else 0.0      # (A) then lets own particles stray H from their slab
    made = halo.partition_scene(gbuf, world, depth, contact_reach=reach)
    outs = []
    for guard in (True, False):
        bus, exs, engs = ranks(sb, made, mode, guard=guard, path=path, bounds=bounds)
        for _ in range(3):
            frame(bus, exs, engs)
        if guard:
            assert all(e.info("halo_guard") == 1 and e.halo_guard_status().kinds == 0 for e in engs)
            assert all(e.info("halo_guard_refreshes") >= 3 * 64 // depth for e in engs)
        else:
            assert all(e.info("halo_guard") == 0 for e in engs)
        if mode == 0 and path == 2:
            assert any(e.info("substeps_per_launch") > 1 for e in engs)      # the blocked kernel ran
        outs.append([e.load_buffers(lbuf.copy()) for e, (lbuf, _) in zip(engs, made)])
        destroy(engs)
    for a, b in zip(*outs):
        assert a.particles.tobytes() == b.particles.tobytes() and a.beams.tobytes() == b.beams.tobytes()


def test_collisions_off_clouds_pass_through_quietly(sb):
    """Without contacts only (C) and (D) apply: the clouds fly through each other, no raise, bit-exact."""
    from test_partition_cpu import two_clouds
    halo = sb.halo
    frames = 9
    gbuf = two_clouds(sb)
    want = single_frames(sb, gbuf, frames, mode=0)[-1]
    made = halo.partition_scene(gbuf, 2, CLOUD_DEPTH)
    bus, exs, engs = ranks(sb, made, 0)
    for _ in range(frames):
        frame(bus, exs, engs)
    assert np.array_equal(gather(made, engs, gbuf.particle_count).view("u4"), want.view("u4"))
    assert all(e.halo_guard_status().refreshes == frames * 64 for e in engs)
    destroy(engs)


def test_peer_exchanger_raises_too(sb):
    """In-process PeerExchangers (sb_peer_exchange runs the guard behind its unpack), guarded: RepartitionDue on the clouds."""
    from test_partition_cpu import two_clouds
    halo = sb.halo
    gbuf = two_clouds(sb)
    made = halo.partition_scene(gbuf, 2, CLOUD_DEPTH, contact_reach=CLOUD_REACH)
    engs = [engine_for(sb, lbuf, 1) for lbuf, _ in made]      # all-pairs: calls only enqueue (no rank waits for the other)
    exs = [halo.PeerExchanger(e, plan, timeout_ms=3000, guard=True) for e, (_, plan) in zip(engs, made)]
    cards = [ex.card for ex in exs]
    for ex in exs:
        ex.connect(cards)
    raised = []
    for f in range(9):
        for ex in exs:
            try:
                ex.frame()
            except halo.RepartitionDue as exc:
                raised.append((f, exc.rank, exc.kinds))
        if raised:
            break
    assert raised and all(k & (SLAB | BAND) for _, _, k in raised), raised
    destroy(engs)


def test_guard_argument_and_state_errors(sb):
    from test_partition_cpu import two_clouds
    halo = sb.halo
    E = sb.engine.EngineError
    gbuf = two_clouds(sb)
    made = halo.partition_scene(gbuf, 2, CLOUD_DEPTH, contact_reach=CLOUD_REACH)
    lbuf, plan = made[0]
    g = plan.guard
    own = plan.owned_particles
    eng = engine_for(sb, lbuf)
    args = lambda **kw: dict(dict(rank=0, world=2, depth=1, contact_reach=g.reach, hop=g.hop, lo=g.lo, hi=g.hi,  # noqa: E731
                                  own_particles=own, held=g.held[own]), **kw)
    with pytest.raises(E, match="before sb_halo_configure") as ei:
        eng.halo_guard(**args())
    assert ei.value.status == 5
    with pytest.raises(E, match="without a guard"):
        eng.halo_guard_status()
    eng.halo_configure(*plan.lists())
    eng.halo_guard(**args())
    assert eng.info("halo_guard") == 1 and eng.halo_guard_status().refreshes == 0
    for kw, status in ((dict(world=65, lo=np.zeros(65), hi=np.zeros(65)), 6), (dict(rank=2), 1), (dict(depth=0), 1),
                       (dict(contact_reach=80.0), 1), (dict(motion=16.0), 1), (dict(hop=float("nan")), 1),
                       (dict(own_particles=np.array([lbuf.particle_count + 3], "u4"), held=np.zeros(1, "u8")), 1)):
        with pytest.raises(E) as ei:
            eng.halo_guard(**args(**kw))
        assert ei.value.status == status, kw
    assert eng.info("halo_guard") == 0                           # a refused call leaves no guard behind
    eng2 = engine_for(sb, lbuf, 0)                               # collisions off: R does not matter
    eng2.halo_configure(*plan.lists())
    eng2.halo_guard(**args(contact_reach=0.0))
    eng2.write_buffers(lbuf)                                     # a new upload clears the guard ...
    assert eng2.info("halo_guard") == 0
    with pytest.raises(E, match="before sb_halo_configure"):
        eng2.halo_guard(**args())
    eng2.halo_configure(*plan.lists())
    eng2.halo_guard(**args())
    eng2.halo_configure(*plan.lists())                           # ... and so does a new configuration
    assert eng2.info("halo_guard") == 0
    eng2.halo_guard(**args())
    eng2.halo_guard_off()
    assert eng2.info("halo_guard") == 0
    eng.destroy()
    eng2.destroy()
    _, splan = halo.slab_scene(sb, 0, 2, 8, 4, depth=2)
    sbuf, _ = halo.slab_scene(sb, 0, 2, 8, 4, depth=2)
    e3 = engine_for(sb, sbuf, 0)
    with pytest.raises(ValueError, match="slab_scene"):
        halo.Exchanger(e3, splan, None, guard=True)
    e3.destroy()
