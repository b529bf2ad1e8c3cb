"""The conditions that keep tests/test_gpu_gate_edges.py honest, on the ORACLE alone (no GPU): every case of tests/gate_cases.py
stays finite at every checkpoint in every collision mode it is compared in, and bites -- counted in binary32 from the oracle's
READ states, something lies outside the gate the case names, and in the mixed cases at least 64 times as many lie inside it.
Each case prints how many items lay inside and outside each of its gates (pytest -rP shows them)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gate_cases as gc  # noqa: E402

NAMES = gc.NAMES


@pytest.fixture(scope="module")
def cases(sb):
    return {c["name"]: c for c in gc.all_cases(sb)}


def oracle_modes(c):
    """Every collision scan the GPU tests compare this case with."""
    return sorted(set(gc.ref_mode(m) for m in c["modes"]) | ({gc.ALLPAIRS} if c["batch"] else set()))


def test_the_case_list_covers_every_gate(cases):
    assert sorted(cases) == sorted(NAMES)
    named = set()
    for c in cases.values():
        named |= set(c["gates"])
    assert named == {"beam len2", "blocked 1/length", "mirrored", "contact d2", "contact dist", "drag v2"} == set(gc.GATES)
    for c in cases.values():
        P = c["buf"].particle_count
        assert P <= 482 and max(c["checkpoints"]) <= 23


@pytest.mark.parametrize("name", NAMES)
def test_case_is_finite_and_bites(sb, oracle, cases, name):
    c = cases[name]
    bitten = {g: False for g in c["gates"]}
    for mode in oracle_modes(c):
        assessed = [g for g in c["gates"] if not ((g.startswith("contact") and mode == gc.OFF) or
                                                   (g in ("mirrored", "blocked 1/length") and mode != gc.OFF))]
        if not assessed:                                    # (the batch's scan of a case whose gate runs without one: finite is all)
            for n, st in gc.oracle_states(oracle, c, mode).items():
                assert np.isfinite(st.particles[:st.particle_count]).all(), "%s, mode %d: not finite after %d substeps" % (name, mode, n)
            continue
        states, reads = gc.oracle_states(oracle, c, mode, reads=True)
        for n, st in states.items():
            assert np.isfinite(st.particles[:st.particle_count]).all(), "%s, mode %d: not finite after %d substeps" % (name, mode, n)
            B = st.beam_count
            rec = st.beams[st.mapping[st.max_particles:st.max_particles + B].astype(np.int64)]
            for f in ("target_length", "last_length", "strain", "stress"):
                assert np.isfinite(rec[f]).all(), "%s, mode %d: beam %s not finite after %d substeps" % (name, mode, f, n)
        got = c["bite"](reads, contacts=mode != gc.OFF)
        notes = got.pop("notes")
        print("%s, oracle mode %d, %d substeps: %s; %s" % (name, mode, len(reads), "; ".join(
            "%s: %d inside, %d outside" % (g, i, o) for g, (i, o) in got.items()) or "control (no gate named)", notes))
        for g, (inside, outside) in got.items():
            if g not in assessed:
                continue                                    # no collision scan in this run / the blocked kernel runs without one
            if outside:
                bitten[g] = True
            if c["mixed"]:
                assert outside >= 1 and inside >= 64 * outside, (name, mode, g, inside, outside)
        if name.startswith("M2 spring 1200") and mode == gc.OFF:
            assert notes["f_30_31"] >= 1 and notes["f_sat"] == 0, notes
        if name.startswith("M2 spring 2e+29") and mode == gc.OFF:
            assert notes["f_sat"] >= 1, notes
        if name.startswith("M1") and mode == gc.OFF:
            assert notes["len2_zero"] >= 1, notes
        if name.startswith("M3"):
            assert notes["v2_subnormal"] >= 5, notes
        if "contact dist" in c["gates"] and mode != gc.OFF:
            assert notes["contacts_outside_dist"] >= 1, notes
        if name.startswith("M4"):                           # ordinary contacts beside the offender, in the population the gate ballots
            assert notes["contacts_inside_dist"] >= 64 * notes["contacts_outside_dist"] >= 64, notes
    assert all(bitten.values()), (name, bitten)


def test_m3_speeds_are_what_they_are_meant_to_be(cases):
    """(1e-25)^2 underflows to zero in binary32: those five particles move and still have v2 == 0; the five at 1e-21 have a
    subnormal v2; five are at rest."""
    buf = cases["M3 drag exponent 2"]["buf"]
    v = buf.particles[:, 2:4]
    v2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
    assert (v2[list(gc.M3_TINY)] == 0).all() and (v[list(gc.M3_TINY)] != 0).all()
    assert ((v2[list(gc.M3_SUBNORMAL)] > 0) & (v2[list(gc.M3_SUBNORMAL)] < np.float32(2.0) ** -126)).all()
    assert (v[list(gc.M3_REST)] == 0).all()
    rest = np.setdiff1d(np.arange(buf.particle_count), gc.M3_TINY + gc.M3_SUBNORMAL + gc.M3_REST)
    assert gc.in_range(v2[rest], gc.SQRT_LO, gc.SQRT_HI).all()
