"""The scene tables the engine's four whole-scene reports share (csrc/sb_report.hip sbq_need): one engine asked all four in
changing orders across three uploads gives, byte for byte, what fresh engines give that follow the same uploads and frames and
only ever call one report -- so no report reads a table another built for an earlier scene, and none builds the shared part again."""
import numpy as np
import pytest

import report_harness as rh
from test_gpu_parity import OFF, TILED
from test_gpu_reupload import without

pytestmark = pytest.mark.gpu

MAXP, MAXB, BOUNDS = 128, 320, 1000.0
KEYS = {r: r + "_table_build_us" for r in ("summary", "bodies", "contacts", "body_summary")}


def report(eng, which):
    """the report's outputs as bytes"""
    out = {"summary": lambda: eng.summary(counts=True), "bodies": lambda: eng.bodies(sizes=True), "contacts": lambda: eng.contacts(pairs=64),
           "body_summary": lambda: eng.body_summary(rows=8, counts=True, rank=True)}[which]()
    return tuple(t.cpu().numpy().tobytes() for t in out)


def uploads(sb):
    first = sb.scenes.default_buffers(2, MAXP, MAXB)
    keep = np.ones(first.beam_count, bool)
    keep[np.random.default_rng(5).choice(first.beam_count, max(first.beam_count // 100, 1), replace=False)] = False   # ~1 % removed
    p, b = sb.scenes.rectangle(200.0, 300.0, 30.0, 8, 6, 50.0, 700.0, 0.2, 1.0e9, anti_diagonal=False, layout=2)
    pv = np.zeros((p.shape[0], 6), "<f4")
    pv[:, :2] = p
    other = sb.scenes.Buffers(2, MAXP, MAXB)     # an 8 x 6 lattice at the engine's capacity: another scene altogether
    other.set_scene(pv, b)
    return [(first, 2, ("body_summary", "contacts", "summary", "bodies")),
            (without(first, keep), 1, ("bodies", "summary", "contacts", "body_summary")),
            (other, 1, ("contacts", "summary", "bodies", "body_summary"))]


@pytest.mark.parametrize("kw", [{}, {"path": TILED}], ids=["default path", "tiled"])
def test_reports_share_tables_in_any_order(sb, kw):
    """A report's *_table_build_us is the build time of the shared parts its call asked for plus its private table (summary's
    beam leaves; body summary's fourth beam plane where bodies built the other three before it), latched at the call.  Any build of
    the particle part clocks a new time for it and drops the beam part, so "after the round's first report nobody builds the
    particle part again" is: every report, called a second time once the round is over, still reports the figure it latched at
    its first call.  Contacts' key is the particle part alone, a lower bound of the other three; bodies' is one of body summary's,
    and the same value where body summary built all four planes in one pass before bodies ran."""
    plan = uploads(sb)
    eng = sb.Engine(bounds_size=BOUNDS, layout=2, max_particles=MAXP, max_beams=MAXB, collision_mode=OFF, **kw)
    got = []
    for n, (buf, frames, order) in enumerate(plan):
        eng.write_buffers(buf)
        for _ in range(frames):
            eng.frame()
        out, us = {}, {}
        for which in order:
            out[which] = report(eng, which)
            us[which] = eng.info(KEYS[which])
        assert all(v > 0 for v in us.values()), us
        assert us["contacts"] <= min(us["summary"], us["bodies"]), us
        assert us["bodies"] <= us["body_summary"], us
        if order.index("body_summary") < order.index("bodies"):
            assert us["bodies"] == us["body_summary"], us
        for which in order:                                                              # every report again ...
            assert report(eng, which) == out[which], (which, "upload", n)
            assert eng.info(KEYS[which]) == us[which], (which, "upload", n, us)          # ... and nothing was built since its first call
        got.append(out)
    assert eng.info("uploads_edited") == 1      # the second upload kept the plan: the caller's slots are a subset of the engine's
    eng.destroy()
    for which in KEYS:
        alone = rh.engine(sb, plan[0][0], BOUNDS, collision_mode=OFF, **kw)
        for n, (buf, frames, order) in enumerate(plan):
            if n:
                alone.write_buffers(buf)
            for _ in range(frames):
                alone.frame()
            assert report(alone, which) == got[n][which], (which, "upload", n)
        alone.destroy()
