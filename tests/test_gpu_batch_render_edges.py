"""sb_batch_render_device at the hand-built scenes of tests/render_cases.py, one per scene of one batch: the cases of
tests/test_gpu_render_edges.py, here with the beam clip running against a band's rows.  Far-off and non-finite positions are
written with write_particles_device.  Every picture is compared with np.array_equal against render_ref of what load_scene returns:
at 64^2 (one band) and at 256^2 (several), with the case's own bounds and radius, and the far-off beams also with a second bounds
and radius that move the crossings to other bands.  The batch has no counter of its wave lists: that the cases hit their
thresholds is asserted on the CPU (tests/test_render_cases_cpu.py)."""
import numpy as np
import pytest

import render_cases as rc
from test_gpu_batch_render import Refs

pytestmark = pytest.mark.gpu
CAP = (272, 528)   # the largest case (the shuffled default scene in 256 / 512) and some slack
FAR = ("far_beams", "far_beams_twin", "far_miss", "far_miss_twin", "far_n_2p53")
SECOND = (200.0, 4.0)   # the second bounds and radius of the far-off beams


@pytest.fixture(scope="module", params=[1, 2])
def batch(sb, request):
    """One batch per layout, a case per scene, far-off and non-finite positions imported on the device."""
    import torch
    layout = request.param
    names = [n for n, c in rc.CASES.items() if layout in c.layouts]
    bufs = [rc.refit(sb, rc.CASES[n].buffers(sb, layout), *CAP) for n in names]
    be = sb.BatchEngine(n_scenes=len(names), layout=layout, max_particles=CAP[0], max_beams=CAP[1], collision_mode=0)
    for i, (n, b) in enumerate(zip(names, bufs)):
        be.write_scene(rc.benign(b) if rc.CASES[n].device_positions else b, i, 1)
    p, _, _ = be.state_tensors()
    for i, (n, b) in enumerate(zip(names, bufs)):
        if rc.CASES[n].device_positions:
            p[i, :, :2] = torch.from_numpy(np.ascontiguousarray(b.particles[:, :2])).to(p.device)
    be.write_particles_device(p)
    be.sync()
    for i, (n, b) in enumerate(zip(names, bufs)):          # the read-back holds every case's own positions, bit for bit
        got = be.load_scene(i, b.copy())
        idx = b.mapping[:b.particle_count].astype(np.int64)
        assert np.array_equal(got.particles[idx, :2].view(np.uint32), b.particles[idx, :2].view(np.uint32)), n
    yield be, names, bufs, Refs()
    be.destroy()


def one(be, refs, i, buf, res, S, r, what):
    got = be.render(res, bounds_size=S, particle_radius=r, first=i, count=1)
    be.sync()
    g = got.cpu().numpy()[0]
    want = refs.picture(be, i, buf, res, S, r)
    bad = int((g != want).any(axis=-1).sum())
    print("%s at %d^2 (%g, %g): %d pixels differ, %d not black" % (what, res, S, r, bad, int(want.any(axis=-1).sum())))
    assert np.array_equal(g, want), "%s at %d^2 (%g, %g): %d pixels differ" % (what, res, S, r, bad)
    return g


@pytest.mark.parametrize("res", [64, 256])
def test_every_case_with_its_own_bounds_and_radius(batch, res):
    be, names, bufs, refs = batch
    for i, (n, b) in enumerate(zip(names, bufs)):
        _, S, r = rc.CASES[n].renders[0]
        g = one(be, refs, i, b, res, S, r, n)
        if res == rc.CASES[n].renders[0][0]:
            assert g.any() != rc.CASES[n].nothing, n
        assert (be.info("render_bands") == 1) == (res == 64)
    st = be.load_scene(names.index("nonfinite_colours"), bufs[names.index("nonfinite_colours")].copy())
    assert np.isnan(st.beams["strain"][0]) and np.isinf(st.beams["stress"][4])          # the reference did see them


@pytest.mark.parametrize("res", [64, 256])
def test_far_beams_at_a_second_bounds_and_radius(batch, res):
    """Another bounds moves every crossing (toPx scales by res / bounds) and, at 256^2, into other bands."""
    be, names, bufs, refs = batch
    S2, r2 = SECOND
    for n in FAR + ("nonfinite_particles",):
        i = names.index(n)
        _, S, r = rc.CASES[n].renders[0]
        a = one(be, refs, i, bufs[i], res, S, r, n)
        b = one(be, refs, i, bufs[i], res, S2, r2, n + ", second bounds")
        assert (be.info("render_bands") == 1) == (res == 64)
        if n in ("far_beams", "far_beams_twin"):
            assert a.any() and b.any() and not np.array_equal(a, b)
            if res == 256:                                  # they differ in most rows, so in most bands: other bands draw the beams
                assert int((a != b).any(axis=(1, 2)).sum()) > res // 2


def test_the_whole_batch_in_one_launch(batch):
    """Every scene in one launch, at the batch's own bounds and radius, at 64^2 and 256^2."""
    from test_gpu_batch_render import assert_pictures
    be, names, bufs, refs = batch
    for res in (64, 256):
        assert_pictures(be, bufs, res, refs, "edge cases, one launch", prefill=0xAB)
        assert (be.info("render_bands") == 1) == (res == 64)
