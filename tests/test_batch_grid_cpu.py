"""The batch's contact cells without a GPU: the option's ABI and validation, and that the scenes of tests/batch_grid_cases.py bite --
the oracle alone runs every finite one to the end, and on the pile it shows contacts enough for more than one selection sweep and
cells fuller than a bucket (so the GPU tests exercise the sweeps and the overflow fallback, not only the easy path)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
import batch_grid_cases as gc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def default_options(sb):
    L = sb.batch.load_library()
    o = sb.batch.SbBatchOptions()
    L.sb_batch_default_options(ctypes.byref(o))
    return L, o


def test_option_struct_keeps_its_size_against_gcc(sb, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "softbody.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(sb_batch_options), offsetof(sb_batch_options, grid_min_particles), offsetof(sb_batch_options, reserved)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off, res = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    O = sb.batch.SbBatchOptions
    assert size == ctypes.sizeof(O) == 64                      # what it was before the field was carved from `reserved`
    assert off == O.grid_min_particles.offset == 40 and res == O.reserved.offset == 44


def test_default_options_leave_the_threshold_zero(sb):
    L, o = default_options(sb)
    assert o.grid_min_particles == 0 and list(o.reserved) == [0] * 5 and o.collision_mode == 2


@pytest.mark.parametrize("value", [1025, 4096, 0xFFFFFFFE])
def test_a_threshold_that_is_no_particle_count_is_invalid_before_a_device_is_looked_for(sb, value):
    L, o = default_options(sb)
    o.grid_min_particles = value
    h = ctypes.c_void_p()
    assert L.sb_batch_create(ctypes.byref(o), ctypes.byref(h)) == 1
    msg = L.sb_batch_last_error(None)
    assert b"grid_min_particles" in msg and str(value).encode() in msg, msg
    assert not h.value


@pytest.mark.parametrize("value", [None, 0, 1, 128, 1024, gc.NEVER])
def test_a_documented_threshold_passes_validation(sb, value):
    """Accepted: without a GPU the error is the missing device's (status 3, not SB_ERR_INVALID) and the test ends there; with
    one the batch exists and reports the resolved value.  (That an unknown info key is still named needs a batch, so on a
    machine without a GPU only tests/test_gpu_batch_grid.py checks it.)"""
    import torch
    try:
        be = sb.BatchEngine(n_scenes=1, max_particles=128, max_beams=8, grid_min_particles=value)
    except sb.EngineError as e:
        assert not torch.cuda.is_available() and e.status == 3, e
        return
    assert be.info("grid_min_particles") == (value or be.info("grid_min_particles")) > 0
    with pytest.raises(sb.EngineError) as ei:
        be.info("no_such_key")
    assert "no_such_key" in str(ei.value)                      # an unknown key is still named
    be.destroy()


def test_every_finite_case_keeps_the_oracle_finite(sb, oracle):
    for case in gc.finite_cases(sb):
        def finite(refs, k, case=case):
            for i, ref in enumerate(refs):
                assert np.isfinite(gc.positions(ref)).all(), "%s: scene %d is not finite after op %d" % (case["name"], i, k)
        gc.run_oracles(oracle, case, finite)


def test_the_edge_scene_is_what_it_says(sb):
    pts, idx = gc.edge_points()
    g, cell = gc.cell_geometry(1000.0, 10.0, gc.EDGE_CAP[0])
    q = pts / cell                                             # float32, as the kernel divides
    on = (q == np.floor(q)) & (q > 0)
    assert on[:, 0].sum() >= 3 and on[:, 1].sum() >= 3         # exactly on a border (where k * cell / cell comes back as k)
    d = pts[None, :, :] - pts[:, None, :]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype("f4"))[np.triu_indices(len(pts), 1)]
    assert (dist == np.float32(20.0)).sum() >= 2               # no contact, by a hair
    assert (dist == np.nextafter(np.float32(20.0), np.float32(0))).sum() + ((dist < 20) & (dist > 19.9999)).sum() >= 2
    assert ((dist > 20) & (dist < 20.0001)).sum() >= 2
    assert (dist == 0).sum() == 15                             # six on one spot
    assert (pts[:, 0] == 0).any() and (pts[:, 0] == 1000).any()
    assert not np.array_equal(idx, np.arange(len(idx)))        # the tie-break's data indices are not the slots


def test_geometry_table(sb):
    """What the GPU test expects info("contact_cells_per_side") to say, from the documented rule."""
    cells = [gc.cell_geometry(b, r, gc.GEOMETRY_CAP[0])[0] for b, r in gc.GEOMETRIES]
    assert gc.cell_cap(256) == 25 and gc.cell_cap(128) == 17 and gc.cell_cap(1024) == 50
    assert cells[0] == 25 and cells[1] == 25 and cells[2] == 1 and cells[3] == 4 and cells[4] in (24, 25), cells
    assert gc.cell_geometry(1000.0, 10.0, 1024)[0] == 49 and gc.cell_geometry(1000.0, gc.R_INTEGER, 1024)[0] in (39, 40)


def test_the_pile_bites(sb, oracle):
    """At the checkpoints of the pile's program (start, after the frame, after the 5 substeps), from the oracle's positions."""
    case = gc.case_pile(sb)
    states = [case["bufs"][0].particles[:256, :2].astype("f4").copy()]
    gc.run_oracles(oracle, case, lambda refs, k: states.append(gc.positions(refs[0]).copy()))
    assert len(states) == 3 and all(np.isfinite(s).all() for s in states)
    cell = gc.cell_rule(10.0)
    most_contacts, fullest, touched = 0, 0, np.zeros(256, bool)
    for p in states:
        d = p[None, :, :] - p[:, None, :]
        dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype("f4"))
        contact = (dist < np.float32(20.0)) & ~np.eye(256, dtype=bool)
        most_contacts = max(most_contacts, int(contact.sum(1).max()))
        touched |= contact.any(1)
        cx, cy = (np.clip(np.floor(p[:, a] / cell), 0, 48).astype(int) for a in (0, 1))
        fullest = max(fullest, int(np.bincount(cy * 49 + cx).max()))
    assert most_contacts >= 5, most_contacts                   # more than the four one selection sweep takes
    assert fullest > gc.CELL_K, fullest                        # a bucket overflows: the fallback is due
    assert touched.mean() >= 0.30, touched.mean()


def test_the_rings_are_what_they_say(sb):
    """On the numpy reference of the contacts tests alone: the centre of scene n has exactly its k partners, and before the
    first substep no cell of an uncrowded scene holds more than a bucket does, while the crowded scene's cell holds all ten."""
    import batch_contacts_ref as cr
    case = gc.case_rings(sb)
    g, cell = gc.cell_geometry(1000.0, 10.0, gc.RING_CAP[0])
    assert g == 12 and gc.CELL_K == 4 and len(case["bufs"]) == 9
    assert [k for k, _ in gc.ring_scenes()] == [0, 1, 3, 4, 5, 7, 8, 9, 9]
    for n, ((k, crowded), buf) in enumerate(zip(gc.ring_scenes(), case["bufs"])):
        centre = gc.ring_points(k, crowded, n)[1]
        idx, touch = cr.touching(buf, 10.0)
        assert buf.particle_count == k + 1 and int(touch[centre].sum()) == k, (n, k, touch.sum(1))
        assert not np.array_equal(np.argsort(idx), np.arange(k + 1)) or k < 2          # data indices are not in slot order
        p = buf.particles[idx, :2]
        cx, cy = (np.clip(np.floor(p[:, a] / cell), 0, g - 1).astype(int) for a in (0, 1))
        assert np.abs(p / cell - np.round(p / cell)).min() * cell > 0.25, n          # nobody close enough to a border to be binned otherwise
        load = np.bincount(cy * g + cx)
        if crowded:
            assert load.max() == k + 1 > gc.CELL_K
        else:
            assert load.max() <= gc.CELL_K and (k < 3 or np.count_nonzero(load) >= 3), (n, load[load > 0])
