"""numpy restatement of the halo guard's rule (include/softbody.h sb_halo_guard) -- TEST INFRASTRUCTURE.

The device evaluates the rule in float32 in a fixed order; this does the same operations on np.float32 scalars and arrays,
so the two agree exactly: kinds, violation count and first offending item."""
import numpy as np

SLAB, BAND, BEAM, MOTION = 1, 2, 4, 8
f32 = np.float32


def live_beams(buf):
    """per beam data index of a read-back Buffers: is the beam still in the mapping?"""
    live = np.zeros(buf.max_beams, bool)
    live[buf.mapping[buf.max_particles:buf.max_particles + buf.beam_count].astype(np.int64)] = True
    return live


def thresholds(plan, collide, motion=0.0):
    """(a_lo, a_hi, b_lo[world], b_hi[world], lmax, s) exactly as sb_halo_guard computes them; raises ValueError where the
    engine returns SB_ERR_INVALID."""
    g = plan.guard
    H, R, D = f32(g.hop), f32(g.reach), f32(max(plan.depth, 1))
    s = H / (f32(16.0) * D) if motion == 0 else f32(motion)
    if not (s >= 0 and s <= f32(0.5) * H):
        raise ValueError("motion allowance")
    C = D * (H + s)
    lmax = H - (f32(2.0) * D) * s
    if not lmax > 0:
        raise ValueError("no room for a beam")
    a, b = R - f32(3.0) * C, R - C
    if collide and plan.world > 1 and not a >= 0:
        raise ValueError("R < 3C")
    return (g.lo[plan.rank] - a, g.hi[plan.rank] + a, g.lo - b, g.hi + b, lmax, s)


def sound_reach(hop, depth, motion=0.0):
    """a contact reach the rule accepts for this hop length and depth (3C, plus one)"""
    H, D = f32(hop), f32(depth)
    s = H / (f32(16.0) * D) if motion == 0 else f32(motion)
    return float(f32(3.0) * (D * (H + s))) + 1.0


class GuardModel:
    """One rank's guard.  `particles` = the rank's local particle rows (local data index order, float32 (n, 6)), as
    load_buffers returns them; `beams` = its local beam records (for the endpoints)."""

    def __init__(self, plan, collide, particles, beams, motion=0.0):
        self.plan, self.collide = plan, collide and plan.world > 1     # one rank holds everything: (A), (B) are moot
        self.a_lo, self.a_hi, self.b_lo, self.b_hi, self.lmax, self.s = thresholds(plan, collide, motion)
        self.own = plan.owned_particles.astype(np.int64)
        self.own_b = plan.owned_beams.astype(np.int64)
        self.held = plan.guard.held[self.own]
        self.xprev = np.asarray(particles, f32)[self.own, 0].copy()
        self.ends = (np.asarray(beams["a"], np.int64)[self.own_b], np.asarray(beams["b"], np.int64)[self.own_b])
        self.refreshes = 0
        self.kinds, self.violations, self.first = 0, 0, None      # first = (refresh, is_beam, local data index)

    def refresh(self, particles, n_substeps, live_beams=None):
        """One refresh after n_substeps substeps (on the refreshed state); returns the SB_GUARD_* bits of this refresh.
        live_beams: per local beam data index, False for a beam a delete pass removed (not checked); None: all live."""
        p = np.asarray(particles, f32)
        x = p[self.own, 0]
        kinds_p = np.zeros(x.size, np.uint32)
        with np.errstate(invalid="ignore", over="ignore"):
            if self.collide:
                kinds_p |= np.where(~((x >= self.a_lo) & (x <= self.a_hi)), SLAB, 0).astype(np.uint32)
                for t in range(self.plan.world):
                    if t == self.plan.rank:
                        continue
                    hit = (((self.held >> np.uint64(t)) & np.uint64(1)) == 0) & (x >= self.b_lo[t]) & (x <= self.b_hi[t])
                    kinds_p |= np.where(hit, BAND, 0).astype(np.uint32)
            allow = f32(n_substeps) * self.s
            kinds_p |= np.where(~(np.abs(x - self.xprev) <= allow), MOTION, 0).astype(np.uint32)
            a, b = self.ends
            dx, dy = p[b, 0] - p[a, 0], p[b, 1] - p[a, 1]
            long_ = ~(np.sqrt(dx * dx + dy * dy) <= self.lmax)
            if live_beams is not None:
                long_ &= np.asarray(live_beams, bool)[self.own_b]
            kinds_b = np.where(long_, BEAM, 0).astype(np.uint32)
        self.xprev = x.copy()
        r = self.refreshes
        self.refreshes += 1
        bad_p, bad_b = np.nonzero(kinds_p)[0], np.nonzero(kinds_b)[0]
        here = int(np.bitwise_or.reduce(np.concatenate([kinds_p, kinds_b]))) if kinds_p.size + kinds_b.size else 0
        self.kinds |= here
        self.violations += bad_p.size + bad_b.size
        if self.first is None and (bad_p.size or bad_b.size):
            if bad_p.size:
                self.first = (r, False, int(self.own[bad_p].min()))
            else:
                self.first = (r, True, int(self.own_b[bad_b].min()))
        return here

    def matches(self, status):
        """does an engine.GuardStatus say exactly what this model says?"""
        first = None if status.first_refresh is None else (status.first_refresh, status.first_is_beam, status.first_index)
        return (status.kinds, status.violations, status.refreshes, first) == (self.kinds, self.violations, self.refreshes,
                                                                             self.first)
