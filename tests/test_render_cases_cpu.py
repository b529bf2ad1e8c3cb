"""tests/render_cases.py on the CPU: render_ref's two beam routes against each other, the new cases against host/render.js where it
can walk them, and every case against what its name says, from render_ref's own numbers (particle_boxes, beam_spans)."""
import numpy as np
import pytest

import render_cases as rc
from render_ref import TWO53, WINDOW_THRESHOLD, beam_spans, particle_boxes, render_ref, v8_hypot
from test_render_ref_cpu import check, needs_node, sbp  # noqa: F401  (sbp: the package fixture)

NEW = [n for n in rc.CASES if n not in ("edges", "slot_order", "slot_order_reversed", "nonfinite_colours", "shuffled_mapping")]


def pictures(sbp, case, layout=None, **kw):
    buf = case.buffers(sbp, layout)
    return buf, [render_ref(buf, res, S, r, **kw) for res, S, r in case.renders]


# ---------------------------------------------------------------- the two routes agree

def random_beams(sbp, seed, count, res, far):
    """Beams of up to a few million points around a res^2 image (bounds == res): crossing it, missing it, grazing its corners, with
    an end inside, axis-parallel."""
    rng = np.random.default_rng(seed)
    pts, bms = [], []
    for i in range(count):
        kind = i % 6
        ins = rng.uniform(0.0, res, 2)
        ang = rng.uniform(0.0, 2.0 * np.pi)
        u = np.array([np.cos(ang), np.sin(ang)])
        la, lb = rng.uniform(0.02, 1.0, 2) * far
        if kind == 0:                                   # crossing: through a point inside
            a, b = ins - la * u, ins + lb * u
        elif kind == 1:                                 # missing: through a point outside, mostly
            out = rng.uniform(-2.0 * res, 3.0 * res, 2)
            a, b = out - la * u, out + lb * u
        elif kind == 2:                                 # grazing a corner, within two pixels either side
            c = np.array([rng.choice([0.0, res]), rng.choice([0.0, res])]) + rng.uniform(-2.0, 2.0, 2)
            a, b = c - la * u, c + lb * u
        elif kind == 3:                                 # an end inside
            a, b = (ins, ins + lb * u) if rng.random() < 0.5 else (ins - la * u, ins)
        elif kind == 4:                                 # horizontal, on a row or beside the image
            y = np.floor(rng.uniform(-3.0, res + 3.0)) + rng.choice([0.0, 0.5])
            a, b = np.array([ins[0] - la, y]), np.array([ins[0] + lb, y])
        else:                                           # vertical
            x = np.floor(rng.uniform(-3.0, res + 3.0)) + rng.choice([0.0, 0.5])
            a, b = np.array([x, ins[1] + la]), np.array([x, ins[1] - lb])
        if rng.random() < 0.5:
            a, b = b, a
        pts += [tuple(a), tuple(b)]
        bms.append((2 * i, 2 * i + 1, float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1))))
    return rc.custom(sbp, 2, pts, bms)


@pytest.mark.parametrize("seed,count,far", [(1, 240, 3.0e3), (2, 60, 3.0e5), (3, 18, 3.0e6)])
def test_routes_agree_on_random_beams(sbp, seed, count, far):
    res = 96
    buf = random_beams(sbp, seed, count, res, far)
    enum = render_ref(buf, res, float(res), 0.3, beam_route="enumerate")
    win = render_ref(buf, res, float(res), 0.3, beam_route="window")
    assert np.array_equal(enum, win)
    spans = beam_spans(buf, res, float(res), beam_route="window")
    hit = sum(s["count"] > 0 for s in spans)
    assert 0.3 * count < hit < 0.9 * count, hit            # beams that cross and beams that miss
    assert enum.any()
    # the spans of the two routes are the same numbers
    for a, b in zip(beam_spans(buf, res, float(res), beam_route="enumerate"), spans):
        assert (a["count"], a["first"], a["last"]) == (b["count"], b["first"], b["last"])


@pytest.mark.parametrize("name", [n for n, c in rc.CASES.items() if c.node])
def test_routes_agree_on_cases(sbp, name):
    """Every case whose beams can be enumerated (those render.js can walk), the scaled-down twins included."""
    case = rc.CASES[name]
    for layout in case.layouts:
        _, enum = pictures(sbp, case, layout, beam_route="enumerate")
        _, win = pictures(sbp, case, layout, beam_route="window")
        _, auto = pictures(sbp, case, layout)
        for e, w, a in zip(enum, win, auto):
            assert np.array_equal(e, w) and np.array_equal(e, a)


# ---------------------------------------------------------------- against render.js

@needs_node
@pytest.mark.parametrize("name", [n for n in NEW if rc.CASES[n].node])
def test_new_cases_against_render_js(sbp, tmp_path, name):
    """Byte for byte, as check does.  The cases render.js cannot finish are not here: far_beams, far_miss, far_n_2p53 (n of 1e14
    and beyond: hours, or no termination at n >= 2^53) and nonfinite_particles (it does not terminate).  For those the reference
    stands on the agreement of its two routes (above: on random beams, and on far_beams_twin / far_miss_twin, which are the same
    geometry at n of a few million and ARE checked against render.js here, through the window route they take by default) and on
    the window route's own assertion about its ends."""
    case = rc.CASES[name]
    for layout in case.layouts:
        buf = case.buffers(sbp, layout)
        for res, S, r in case.renders:
            check(tmp_path, buf, res, bounds_size=S, particle_radius=r)


def test_the_twins_take_the_window_route(sbp):
    for name in ("far_beams_twin", "far_miss_twin"):
        case = rc.CASES[name]
        res, S, _ = case.renders[0]
        spans = beam_spans(case.buffers(sbp), res, S)
        assert all(s["windowed"] and s["n"] + 1 > WINDOW_THRESHOLD for s in spans), name


# ---------------------------------------------------------------- every case hits what its name says

@pytest.mark.parametrize("name", list(rc.CASES))
def test_case_hits_its_edge(sbp, name):
    case = rc.CASES[name]
    for layout in case.layouts:
        buf = case.buffers(sbp, layout)
        res, S, r = case.renders[0]
        pic = render_ref(buf, res, S, r)
        assert pic.any() != case.nothing, "%s: %s" % (name, "drawn" if pic.any() else "black")
        ex = case.expect
        boxes = particle_boxes(buf, res, S, r)
        for slot, pixels in ex.get("boxes", {}).items():
            assert boxes["pixels"][slot] == pixels, (name, slot, boxes["pixels"][slot])
        spans = beam_spans(buf, res, S)
        for slot, count in ex.get("points", {}).items():
            assert spans[slot]["count"] == count, (name, slot, spans[slot])
        for slot, k in ex.get("first", {}).items():
            assert spans[slot]["count"] > 0 and spans[slot]["first"] >= k, (name, slot, spans[slot])
        for slot, (lo, hi) in ex.get("n", {}).items():
            assert lo <= spans[slot]["n"] < hi, (name, slot, spans[slot])
            assert spans[slot]["drawn"] == (spans[slot]["n"] < TWO53)
        for slot in ex.get("undrawn", []):
            assert spans[slot]["count"] == 0, (name, slot, spans[slot])
        for slot, px, py, which in ex.get("ties", []):
            cx, cy = boxes["cx"][slot], boxes["cy"][slot]
            d = float(v8_hypot(np.array([(px + 0.5) / res * S - cx]), np.array([(py + 0.5) / res * S - cy]))[0])
            bound = r if which == "r" else r * 0.8
            assert d == bound, (name, slot, px, py, d, bound)               # bit for bit: both are float64
            want = (0, 0, 0) if which == "r" else (255, 255, 255)           # d < r fails: black; d < 0.8 r fails: the ring
            assert tuple(pic[res - 1 - py, px]) == want, (name, slot, px, py, pic[res - 1 - py, px])


def test_far_beams_are_what_they_claim(sbp):
    case = rc.CASES["far_beams"]
    res, S, r = case.renders[0]
    buf = case.buffers(sbp)
    spans = beam_spans(buf, res, S)
    assert all(s["drawn"] and s["windowed"] and s["count"] > 0 and s["n"] > 1e14 for s in spans)
    assert spans[0]["first"] == 0 and spans[0]["last"] < spans[0]["n"]                         # A inside
    assert spans[1]["last"] == spans[1]["n"]                                                   # B inside
    for s in spans[2:10]:                                                                      # both ends outside
        assert 0 < s["first"] and s["last"] < s["n"]
    P = buf.particles
    d = [(float(P[2 * i + 1, 0]) - float(P[2 * i, 0]), float(P[2 * i + 1, 1]) - float(P[2 * i, 1])) for i in range(len(spans))]
    assert {(np.sign(x), np.sign(y)) for x, y in d[2:6]} == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
    assert abs(d[2][0]) > abs(d[2][1]) and abs(d[3][0]) > abs(d[3][1]) and abs(d[4][0]) < abs(d[4][1]) and abs(d[5][0]) < abs(d[5][1])
    # shallow: the minor axis cuts the interval (fewer points than the x range alone would give); steep likewise
    for i in (2, 3, 4, 5):
        assert spans[i]["count"] < min(spans[i]["nx"], spans[i]["ny"]), (i, spans[i])
    assert d[6][1] == 0.0 and spans[6]["count"] >= res and d[7][0] == 0.0 and spans[7]["count"] >= res
    assert 0 < spans[8]["count"] <= 32 and 0 < spans[9]["count"] <= 32 and spans[2]["count"] > 32   # both draw routes
    assert spans[10]["count"] == 51                                                            # x = 0 .. 50, one point each
    for name in ("far_miss", "far_miss_twin"):                                                 # the two intervals do not meet
        c = rc.CASES[name]
        for s in beam_spans(c.buffers(sbp), c.renders[0][0], c.renders[0][1]):
            assert s["drawn"] and s["nx"] > 0 and s["ny"] > 0 and s["count"] == 0, (name, s)


def test_nonfinite_particles_are_what_they_claim(sbp):
    case = rc.CASES["nonfinite_particles"]
    res, S, r = case.renders[0]
    buf = case.buffers(sbp)
    b = particle_boxes(buf, res, S, r)
    assert abs(b["x0"][9]) >= TWO53 and not b["ok"][9]                       # a box bound of 2^53 px and beyond
    assert 2.0 ** 52 < abs(b["x1"][10]) < TWO53                              # and one just below
    assert not b["ok"][1:7].any() and b["ok"][[0, 7, 11, 12, 13]].all() and 0 < b["pixels"][7] < 9 and b["pixels"][8] == 0
    spans = beam_spans(buf, res, S)
    assert [s["drawn"] for s in spans] == [False] * 6 + [True, True, False, True, True, True, False, True]
    assert all(spans[i]["count"] > 0 for i in (6, 7, 9, 10, 11, 13))
