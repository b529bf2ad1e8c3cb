"""The conditions that keep tests/test_gpu_promise_flags.py honest, on the ORACLE alone (no GPU): every case of
tests/promise_cases.py, stepped one substep at a time over each of its schedules, is finite throughout and walks its flag through
the transitions it is named for.  Each case prints the substeps at which they happen (pytest -rP shows them).  These are
conditions, not measurements: a scene that misses one is changed, not the assertion."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import promise_cases as pc  # noqa: E402

NAMES = pc.NAMES


@pytest.fixture(scope="module")
def cases(sb):
    return {c["name"]: c for c in pc.all_cases(sb)}


def runs_of(trace, what):
    """[(nonempty, first substep, last substep)] of the maximal runs of substeps whose set `what` (1: accelerations, 2: yielded
    beams) is / is not empty."""
    out = []
    for row in trace:
        on = len(row[what]) > 0
        if out and out[-1][0] == on:
            out[-1][2] = row[0]
        else:
            out.append([on, row[0], row[0]])
    return [tuple(r) for r in out]


def test_the_names_are_the_cases_and_they_are_small(cases):
    assert sorted(cases) == sorted(NAMES)
    for c in cases.values():
        assert c["buf"].particle_count == 1920
        for calls in c["schedules"].values():
            assert sum(pc.substeps(x) for x in calls) <= 250
    for K in pc.KS:
        for sched in (pc.SCHEDULE_A, pc.SCHEDULE_B):
            assert {1, 2, K - 1, K, K + 1, 37} <= set(sched)


@pytest.mark.parametrize("name", NAMES)
def test_case_is_finite_and_bites(sb, oracle, cases, name):
    c = cases[name]
    for label, calls in c["schedules"].items():
        edit = pc.a4_edit(c) if "import_particle" in c else None
        states, trace = pc.oracle_run(oracle, c, calls, edit=edit)
        for i, st in enumerate(states):
            assert np.isfinite(st.particles[:st.particle_count]).all(), "%s, schedule %s: not finite behind call %d" % (name, label, i)
            B = st.beam_count
            rec = st.beams[st.mapping[st.max_particles:st.max_particles + B].astype(np.int64)]
            for f in ("target_length", "last_length", "strain", "stress"):
                assert np.isfinite(rec[f]).all(), "%s, schedule %s: beam %s not finite behind call %d" % (name, label, f, i)
        acc, yld = runs_of(trace, 1), runs_of(trace, 2)
        print("%s, schedule %s: accelerations nonzero in substeps %s; beams yielded in substeps %s; beams %s" % (
            name, label, [(a, b) for on, a, b in acc if on], [(a, b) for on, a, b in yld if on], sorted(set(r[3] for r in trace))))
        if name == "A1 bounce":                             # clean -> dirty -> clean -> dirty, the clean stretch longer than any call
            on = [r for r in acc if r[0]]
            assert len(on) >= 2, acc
            between = [r for r in acc if not r[0] and on[0][2] < r[1] < on[1][1]]
            assert between and between[0][2] - between[0][1] + 1 >= 38, acc
            assert not any(len(r[2]) for r in trace), "A1 is meant to move the acceleration flag alone: nothing yields"
            # ... and the schedule LOOKS at it: a call ends inside a contact window, a later one where the accelerations have been
            # zero for two substeps, a later one inside the next window (the checkpoints at which the GPU test asserts the flag)
            ends = np.cumsum([pc.substeps(x) for x in calls])
            dirty = [int(n) for n in ends if len(trace[n - 1][1])]
            clean = [int(n) for n in ends if n >= 2 and not len(trace[n - 1][1]) and not len(trace[n - 2][1])]
            print("%s, schedule %s: calls end in contact after %s substeps, clean for two substeps after %s" % (name, label, dirty, clean))
            assert len(dirty) >= 2 and any(dirty[0] < n < dirty[-1] for n in clean), (label, dirty, clean)
            assert any(n > dirty[-1] for n in clean), (label, dirty, clean)
        if name in ("A2 one corner", "A4 import"):
            ends = np.cumsum([pc.substeps(x) for x in calls])
            assert any(len(trace[n - 1][1]) for n in ends), "no call of schedule %s ends while the corner touches" % label
            first = next(r[1] for r in acc if r[0] and (name == "A2 one corner" or r[1] > 10))
            assert 8 <= first, acc
            corner = set(int(p) for p in c["corner"])
            for row in trace:
                if row[0] >= first:
                    assert len(row[1]), "%s: nobody touches in substep %d" % (name, row[0])
                    assert set(int(p) for p in row[1]) <= corner, (name, row[0], row[1])
        if name == "A4 import":                             # the imported acceleration is the first one, and the substep behind consumes it
            done = sum(calls[:c["import_after_call"] + 1])
            assert all(len(r[1]) == 0 for r in trace if r[0] <= done)
            assert list(pc.acc_set(states[c["import_after_call"]])) == [c["import_particle"]]
            assert len(trace[done][1]) == 0
        if name == "A3 -0.0":
            st0 = states[0]
            assert st0.particles[pc.A3_NEG0, 4:6].view("<u4").tolist() == [0x80000000, 0]
            assert sorted(pc.acc_set(st0)) == sorted([pc.A3_NEG0, pc.A3_PLAIN])
            assert len(pc.acc_set(states[1])) == 0 and len(pc.acc_set(states[2])) == 0
        if "yields" in c:                                   # exactly the intended beams, from the substep the case names on
            lo, hi = c["yield_within"]
            first = next(r[0] for r in trace if len(r[2]))
            assert lo <= first <= hi, (name, first)
            for row in trace:
                assert sorted(int(j) for j in row[2]) == (c["yields"] if row[0] >= first else []), (name, row[0], row[2])
        if "offender" in c:                                 # yield in substep 1, removed by the pass of the first frame, survivors kept
            assert sorted(int(j) for j in trace[0][2]) == sorted(c["offender"] + c["survivors"])
            before = pc.live_beams(c["buf"])
            after = pc.live_beams(states[c["pass_of_call"]])
            assert sorted(before - after) == c["offender"], (name, sorted(before - after))
            for st in states[c["pass_of_call"]:]:
                assert sorted(int(j) for j in pc.yielded(st)) == c["survivors"], name
                assert pc.live_beams(st) == after
            print("%s: beams %s removed by the pass of call %d (a frame), %s survive it yielded" % (name, c["offender"], c["pass_of_call"], c["survivors"]))
