"""Scenes and programs of the summary tests (sb_batch_summary_device).  The scenes are tests/batch_cases.py's and
tests/batch_grid_cases.py's; a case here adds `compare_after`: the indices of the program's ops after which the batch's summary()
is compared with tests/batch_summary_ref.py on one oracle per scene.  tests/test_batch_summary_cpu.py runs the oracle side alone
(no warnings, and that the cases bite), tests/test_gpu_batch_summary.py both sides."""
import numpy as np

import batch_cases as bc
import batch_grid_cases as gc
import batch_summary_ref as sr


def grab_inputs(sb, n, strength=500.0):
    """A hard mouse grab at (300, 450), the same for every scene: it tears the 12 x 12 lattice of case_hetero within 5 substeps."""
    b = sb.Buffers(1, 4, 4)
    b.user_strength = strength
    b.set_user_input(mouse_pos=(300.0, 450.0), mouse_vel=(40.0, 30.0), mouse_active=True)
    return [b.user_input_bytes()] * n


def case_hetero(sb):
    """Capacity 1024 / 4096 (the full-width trees), an empty and a never-uploaded scene; after its program and after step(5).
    Nothing breaks in that run (no beam of these scenes comes near its limit), so a grab and five substeps more follow: break
    flags are pending then (129 in the lattice), mid-frame."""
    c = bc.case_hetero(sb)
    n = len(c["program"])
    c["program"] = c["program"] + [("step", 5), ("inputs", grab_inputs(sb, len(c["bufs"]))), ("step", 5)]
    c["compare_after"] = [n - 1, n, n + 2]
    return c


def case_break(sb):
    """Removed beams, a compacted beam mapping, and (mid-frame) pending flags."""
    c = bc.case_break(sb)
    c["program"] = [("frame", 2), ("step", 5)]
    c["compare_after"] = [0, 1]
    return c


def case_mapping(sb):
    c = bc.case_mapping(sb)
    c["compare_after"] = [len(c["program"]) - 1]
    return c


def case_default_120_300(sb):
    """W = 128 / 512: the smallest power of two at or above the capacity, not the capacity."""
    return dict(name="default scene at 120 / 300", layout=1, cap=(120, 300), mode=bc.ALLPAIRS,
                bufs=[sb.scenes.default_buffers(1, 120, 300)], program=[("frame", 1)], compare_after=[0])


NONFINITE_SCENE = 3   # of case_saturation


def case_saturation(sb):
    """Capacity 8 / 8 (the smallest trees).  The saturation scene clamps its forces and stays finite, so a fourth scene is the
    same one with a NaN coordinate and an infinite velocity: after one substep two of its particles and one of its live beams
    are not finite, and every statistic must leave them out."""
    c = bc.case_saturation(sb)
    bad = c["bufs"][1].copy()
    bad.particles[1, 0] = np.nan
    bad.particles[5, 3] = np.inf
    c["bufs"] = c["bufs"] + [bad]
    c["compare_after"] = [len(c["program"]) - 1]
    return c


def case_pile(sb):
    """256 free discs on the contact cells, mid-frame; max_beams = 0."""
    c = gc.case_pile(sb)
    c["compare_after"] = [len(c["program"]) - 1]
    c["make_oracle"] = gc.make_oracle
    return c


def all_cases(sb):
    return [case_hetero(sb), case_break(sb), case_mapping(sb), case_default_120_300(sb), case_saturation(sb), case_pile(sb)]


def make_oracles(orc, case):
    mk = case.get("make_oracle", bc.make_oracle)
    return [None if b is None else mk(orc, case, b) for b in case["bufs"]]


def expected_rows(orc, case):
    """{op index: [n_scenes, 24] rows} of the case on one oracle per scene, and the oracles at the end."""
    refs, out = make_oracles(orc, case), {}
    for k, op in enumerate(case["program"]):
        bc.apply_to_oracles(refs, op)
        if k in case["compare_after"]:
            out[k] = sr.rows_of(refs, case["bufs"])
    return out, refs
