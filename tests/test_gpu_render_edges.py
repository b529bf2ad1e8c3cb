"""sb_render at the hand-built scenes of tests/render_cases.py: discs and beams at every edge, exact ties of d against r and 0.8 r,
boxes of 64 / 65 pixels and beams of 32 / 33 points (the switch between the per-thread and the per-wave route, asserted through
info "render_wide_particles" / "render_wide_beams"), radius extremes, beams whose ends are 1e15 pixels away (a first inside k of
2^32 and more), n at 2^53, non-finite and far-off particles.  Every comparison is np.array_equal over the whole picture against
render_ref of the state load_buffers returns at that moment.  Nothing is stepped: the engine only holds and draws the state."""
import numpy as np
import pytest

import render_cases as rc
from render_ref import beam_spans, particle_boxes
from test_gpu_parity import OFF
from test_gpu_render import engine, same_picture
from test_gpu_reupload import without

pytestmark = pytest.mark.gpu
ODD = 97   # the odd resolution every case is also drawn at


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def draw(eng, buf, res, S, r, what):
    """The picture against the reference, and the two wave lists against the reference's own counts."""
    _, state = same_picture(eng, buf, 1000.0, res, bounds_size=S, particle_radius=r, what=what)
    wide_p = int((particle_boxes(state, res, S, r)["pixels"] > 64).sum())
    wide_b = sum(s["count"] > 32 for s in beam_spans(state, res, S))
    assert (eng.info("render_wide_particles"), eng.info("render_wide_beams")) == (wide_p, wide_b), what
    return state, wide_p, wide_b


def draw_all(eng, case, buf, what):
    out = []
    for res, S, r in case.gpu_renders:
        out.append(draw(eng, buf, res, S, r, "%s at %d" % (what, res)))
        draw(eng, buf, ODD, S, r, "%s at %d" % (what, ODD))
    return out


def import_positions(eng, buf):
    """The positions of `buf` written over the uploaded ones on the device; the read-back holds them bit for bit."""
    import torch
    t = eng.state_tensors()["particles"]
    t[:, :2] = torch.from_numpy(np.ascontiguousarray(buf.particles[:, :2])).to(t.device)
    eng.write_particles_device(t)
    eng.sync()
    got = eng.load_buffers(buf.copy())
    idx = buf.mapping[:buf.particle_count].astype(np.int64)
    assert np.array_equal(bits(got.particles[idx, :2]), bits(buf.particles[idx, :2]))


CASE_LAYOUTS = [(n, L) for n in rc.CASES for L in rc.CASES[n].layouts]


@pytest.mark.parametrize("name,layout", [(n, L) for n, L in CASE_LAYOUTS if n in rc.UPLOADED])
def test_uploaded_case(sb, name, layout):
    """write_buffers, then render before any step: the upload carries positions, strain and stress."""
    case = rc.CASES[name]
    buf = case.buffers(sb, layout)
    eng = engine(sb, buf, collision_mode=OFF)
    (state, wide_p, wide_b), = draw_all(eng, case, buf, name)[:1]
    res, S, r = case.gpu_renders[0]
    if name == "nonfinite_colours":
        B = buf.beam_count
        for f in ("strain", "stress"):                     # the reference really saw the non-finite values
            assert np.array_equal(bits(state.beams[f][:B]), bits(buf.beams[f][:B])), f
        assert np.isnan(state.beams["strain"][0]) and np.isinf(state.beams["stress"][4])
    ex = case.expect
    if "boxes" in ex:                                      # 64 pixels: its own thread; 65 and more: on the list
        assert wide_p == sum(v > 64 for v in ex["boxes"].values()), (wide_p, ex["boxes"])
    if "points" in ex:
        assert wide_b == sum(v > 32 for v in ex["points"].values()) == 3
    eng.destroy()


@pytest.mark.parametrize("name", rc.IMPORTED)
def test_imported_positions(sb, name):
    """Far-off and non-finite positions: uploaded at benign positions, overwritten on the device, drawn."""
    case = rc.CASES[name]
    layout = case.layouts[-1]
    buf = case.buffers(sb, layout)
    eng = engine(sb, rc.benign(buf), collision_mode=OFF)
    import_positions(eng, buf)
    (state, wide_p, wide_b), = draw_all(eng, case, buf, name)
    res, S, r = case.gpu_renders[0]
    spans = beam_spans(state, res, S)
    if name == "far_beams":                                # crossing beams on the list or not, as their clipped count says
        assert wide_b == sum(s["count"] > 32 for s in spans) >= 6
        assert sum(0 < s["count"] <= 32 for s in spans) >= 2
        assert sum(s["count"] > 32 and s["first"] >= 2 ** 32 for s in spans) >= 3      # the list's high dword is in use
    if case.nothing:
        assert not eng.render(res, S, r).any() and wide_b == 0
    eng.destroy()


@pytest.mark.parametrize("name", ["slot_order", "slot_order_reversed", "discs_64_65_r35", "discs_64_65_r6", "beams_32_33",
                                  "beams_32_33_reversed"])
def test_reuploads(sb, name):
    """A plan-keeping re-upload (the same topology with other colours and velocities) and an upload that cuts one beam: the draw
    tables follow the upload."""
    case = rc.CASES[name]
    buf = case.buffers(sb, 2)
    eng = engine(sb, buf, collision_mode=OFF)
    draw_all(eng, case, buf, name)
    B = buf.beam_count
    again = buf.copy()
    again.beams["strain"][:B] = again.beams["strain"][:B][::-1]
    again.beams["stress"][:B] = -again.beams["stress"][:B]
    again.particles[:, 2:4] = 0.25
    eng.write_buffers(again)
    assert eng.info("uploads_kept") == 1
    draw_all(eng, case, again, name + ", kept plan")
    if B:
        keep = np.ones(B, bool)
        keep[1] = False
        cut = without(again, keep)
        eng.write_buffers(cut)
        state = draw_all(eng, case, cut, name + ", one beam cut")[0][0]
        assert state.beam_count == B - 1
    eng.destroy()
