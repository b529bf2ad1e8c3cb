"""The halo guard without a GPU: the partitioner's guard data (sb_partition_rank_guard) against the plans, and the rule
(tests/halo_guard_ref.py, the numpy restatement of include/softbody.h sb_halo_guard) on oracle-backed simulated ranks --
it must fire no later than the first frame whose owned state leaves the single engine's, and never while the run is
re-partitioned every frame."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from halo_guard_ref import BAND, SLAB, GuardModel, sound_reach, thresholds  # noqa: E402

# The two clouds of test_partition_cpu fly at each other at 20 units per second each.  A guarded run needs R >= 3C with
# C = depth * (H + s); at depth 1 (H = 1.5 * 2r = 30, s = H / 16) that is 95.6, so the reach is 130 here (80 there): still
# no ghosts at the start (the clouds are 224 apart), and a 34-unit leash for (A), more than a frame's flight.
CLOUD_DEPTH, CLOUD_REACH = 1, 130.0


def longest_beam(buf):
    P0 = buf.max_particles
    live = buf.mapping[P0:P0 + buf.beam_count].astype(np.int64)
    a, b = buf.beams["a"][live].astype(np.int64), buf.beams["b"][live].astype(np.int64)
    p = buf.particles
    dx, dy = p[b, 0] - p[a, 0], p[b, 1] - p[a, 1]
    return np.sqrt(dx * dx + dy * dy).max() if live.size else np.float32(0)


@pytest.mark.parametrize("world,depth,reach", [(2, 2, 0.0), (3, 1, 60.0), (4, 2, 150.0)])
def test_guard_data_agrees_with_the_plans(sb, world, depth, reach):
    """held masks: bit t set if and only if rank t holds the particle (own or ghost); lo / hi = the own x-extents; R and H."""
    buf = sb.scenes.default_buffers(2, 256, 512)
    made = sb.halo.partition_scene(buf, world, depth, contact_reach=reach)
    holders = [set(plan.global_particle_id.tolist()) for _, plan in made]
    H = np.float32(1.5) * max(np.float32(20.0), longest_beam(buf))
    for r, (lbuf, plan) in enumerate(made):
        g = plan.guard
        assert g is not None and g.lo.size == world and g.held.size == lbuf.particle_count
        own = plan.owned_particles
        assert g.lo[r] == lbuf.particles[own, 0].min() and g.hi[r] == lbuf.particles[own, 0].max()
        assert np.array_equal(g.lo, made[0][1].guard.lo) and np.array_equal(g.hi, made[0][1].guard.hi)
        assert np.float32(g.reach) == np.float32(reach) and np.float32(g.hop) == H
        for i, gid in enumerate(plan.global_particle_id.tolist()):
            assert int(g.held[i]) == sum(1 << t for t in range(world) if gid in holders[t])
    assert any(int(m) != 1 << r for r, (_, plan) in enumerate(made) for m in plan.guard.held)      # ghosts are in the masks


def test_guard_data_limits(sb):
    from test_partition_cpu import two_clouds
    buf = two_clouds(sb)
    assert all(plan.guard is None for _, plan in sb.halo.partition_scene(buf, 65, 1))              # the guard stops at 64 ranks
    assert all(plan.guard is not None for _, plan in sb.halo.partition_scene(buf, 64, 1))
    with pytest.raises(sb.engine.EngineError, match="particle_radius"):
        sb.halo.partition_scene(buf, 2, 1, particle_radius=0.0)
    _, plan = sb.halo.slab_scene(sb, 0, 2, 8, 4, depth=2)
    assert plan.guard is None


def test_unsound_parameters_are_rejected(sb):
    from test_partition_cpu import two_clouds
    buf = two_clouds(sb)
    (_, plan), _ = sb.halo.partition_scene(buf, 2, CLOUD_DEPTH, contact_reach=CLOUD_REACH)
    thresholds(plan, True)                                              # R = 130 >= 3C = 95.6
    (_, thin), _ = sb.halo.partition_scene(buf, 2, CLOUD_DEPTH, contact_reach=80.0)
    with pytest.raises(ValueError, match="3C"):
        thresholds(thin, True)
    thresholds(thin, False)                                             # without contacts R does not matter
    with pytest.raises(ValueError):
        thresholds(plan, True, motion=16.0)                             # s > H / 2
    assert sound_reach(30.0, 1) == pytest.approx(3 * (30 + 30 / 16) + 1)


class GuardedOracleRank:
    """An OracleRank whose every unpack (the end of a refresh) is checked by a GuardModel, as k_halo_guard does on an engine."""

    def __new__(cls, oracle, lbuf, plan, bounds, mode):
        from halo_oracle import OracleRank

        class Ranked(OracleRank):
            def step(self, n):
                super().step(n)
                self.since_check += n

            def halo_unpack(self, src):
                super().halo_unpack(src)
                self.model.refresh(self._cur(), self.since_check)
                self.since_check = 0

        eng = Ranked(oracle, lbuf, bounds, mode=mode)
        eng.model = GuardModel(plan, mode != 0, lbuf.particles, lbuf.beams)
        eng.since_check = 0
        return eng


def run_clouds(sb, oracle, again, frames=9):
    """(frame at which any rank's guard had fired, or None; frame whose owned state first differs from the single oracle, or
    None; the models of the last partition)"""
    from halo_oracle import LocalBus, OracleRank, frame_all
    from test_partition_cpu import two_clouds
    halo = sb.halo
    world, mode = 2, oracle.COLLIDE_GRID
    gbuf = two_clouds(sb)
    ref = OracleRank(oracle, gbuf, 1000.0, mode=mode)
    wants = []
    for _ in range(frames):
        ref.ref.frame()
        wants.append(ref.load(gbuf).particles.copy())

    def build(made):
        bus, exs, engs = LocalBus(), [], []
        for r, (lbuf, plan) in enumerate(made):
            eng = GuardedOracleRank(oracle, lbuf, plan, 1000.0, mode)
            tr = bus.transport(r, lambda a, b: (np.zeros(max(a, 1), "f4"), np.zeros(max(b, 1), "f4")), lambda t: t)
            exs.append(halo.Exchanger(eng, plan, tr))
            engs.append(eng)
        return bus, exs, engs

    made = halo.partition_scene(gbuf, world, CLOUD_DEPTH, contact_reach=CLOUD_REACH)
    assert all(not plan.peers for _, plan in made)                      # nothing in common at the start
    bus, exs, engs = build(made)
    fired = diverged = None
    P = gbuf.particle_count
    for f in range(frames):
        frame_all(exs, bus, lambda dst, src: dst.__setitem__(slice(None), src))
        if fired is None and any(e.model.kinds for e in engs):
            fired = f
        got = np.zeros_like(wants[f])
        for (lbuf, plan), eng in zip(made, engs):
            out = eng.load(lbuf)
            got[plan.global_particle_id[plan.owned_particles]] = out.particles[plan.owned_particles]
        if diverged is None and not np.array_equal(got[:P].view("u4"), wants[f][:P].view("u4")):
            diverged = f
        if again:
            states = [halo.owned_state(plan, eng.load(lbuf)) for (lbuf, plan), eng in zip(made, engs)]
            made = halo.repartition(gbuf, states, world, CLOUD_DEPTH, CLOUD_REACH)
            bus, exs, engs = build(made)
    return fired, diverged, [e.model for e in engs], made


def test_rule_fires_no_later_than_the_divergence(sb, oracle):
    """Without repartition the clouds fly into each other's slabs: the rule fires (the first refresh that fails is checked
    on the state of that frame), and no later than the first frame whose owned state differs from the single run."""
    fired, diverged, models, _ = run_clouds(sb, oracle, again=False)
    assert diverged is not None and fired is not None and fired <= diverged, (fired, diverged)
    assert any(m.kinds & (SLAB | BAND) for m in models)
    assert all(m.refreshes == 9 * 64 for m in models)                  # a rank without neighbours is checked as well


def test_rule_never_fires_when_repartitioned_every_frame(sb, oracle):
    fired, diverged, models, made = run_clouds(sb, oracle, again=True)
    assert fired is None and diverged is None
    assert sum(p.ghost_p.size for _, plan in made for p in plan.peers) > 40     # the clouds are in each other's zones now
