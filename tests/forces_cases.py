"""Scenes of the engine's forces tests (sb_forces_device) beyond tests/batch_forces_cases.py's, whose scenes run on
one Engine each.  tests/test_forces_cpu.py shows on the restatement alone that they bite; tests/test_gpu_forces.py runs them
through Engine.forces()."""
import numpy as np

import batch_forces_cases as fc

F = np.float32
# data indices of the six particles of permuted_five: the partners' slots 1 .. 5 ascend, their data indices 2, 7, 0, 11, 4 do not
PERMUTED = (9, 2, 7, 0, 11, 4)


def permuted_five(sb, cap=(16, 4)):
    """batch_forces_cases.five_partners -- slot 0 in the middle of five moving partners whose overlaps span three orders of magnitude
    -- under a mapping that is a non-trivial permutation: in ascending DATA-index order the partners come as slots 3, 1, 5, 2, 4.  Six
    lone particles far away fill other data indices."""
    pts = fc.five_partners() + [(50.0 + 60.0 * k, 900.0, 0.0, 0.0) for k in range(6)]
    rest = [d for d in range(cap[0]) if d not in PERMUTED][:6][::-1]
    return fc.scene(sb, cap, pts, data_index=list(PERMUTED) + rest)


def engine_scenes(sb):
    """(name, Buffers, subticks) of every scene of batch_forces_cases' contact and beam cases plus this file's: each fits one Engine
    at bounds 1000, radius 10"""
    out = [("permuted five", permuted_five(sb), 64)]
    for mk, kw in ((fc.case_small, {}), (fc.case_beams, {}), (fc.case_contacts, dict(subticks=64)), (fc.case_contacts, dict(subticks=100)),
                   (fc.case_rings, {}), (fc.case_two_bodies, {})):
        case = mk(sb, **kw)
        for i, buf in enumerate(case["bufs"]):
            if buf is not None:
                out.append(("%s / %d" % (case["name"], i), buf, case.get("subticks", 64)))
    return out


def beam_chain(sb, n_beams, gate=False):
    """n_beams + 1 particles in a row 30 apart, beam j between particles j and j + 1, stretched by 3 %: beam counts on either side of a
    wave and of a workgroup.  gate: every 7th beam's far endpoint is moved 2^50 away in y and every 11th beam has length zero -- lengths
    outside and at the edge of the short sqrt's gate in the same waves as ordinary ones (tests/gate_cases.py's mix)."""
    n = n_beams + 1
    per = 30
    pts = np.zeros((n, 2), "f4")
    pts[:, 0] = 40.0 + 30.9 * (np.arange(n) % per)
    pts[:, 1] = 40.0 + 45.0 * (np.arange(n) // per)
    beams = []
    for j in range(n_beams):
        beams.append((j, j + 1, 30.0, 30.0 + 0.01 * (j % 5), 30.5, 50.0 + j % 3, 700.0))
    if gate:
        for j in range(0, n_beams, 7):
            pts[j + 1, 1] = F(2.0 ** 50)
        for j in range(3, n_beams, 11):
            pts[j + 1] = pts[j]
    rng = np.random.default_rng(n_beams)
    cap = (n + 5, n_beams + 3)
    return fc.scene(sb, cap, pts, beams, data_index=rng.permutation(cap[0])[:n])
