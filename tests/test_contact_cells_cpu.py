"""csrc/sb_contact_cells.h on the host under sanitizers (tests/contact_cells_check.cpp): the contact test, the
cells' rule, the 3 x 3 window over buckets and over sorted runs and the ascending selection, against brute force.  The program
is stand-alone and seeded; this test builds it with `make hostcheck`'s rule and runs it."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "softbody-webgpu_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
           TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_contact_cells_header_against_brute_force_under_sanitizers(san):
    target = os.path.join("hostcheck_build", "contact_cells_check_" + san)
    p = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    r = subprocess.run([os.path.join(CSRC, target)], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    assert "CONTACT_CELLS_CHECK_OK" in r.stdout, r.stdout          # (the program checks its own coverage)


def test_hostcheck_builds_the_program():
    """`make hostcheck` lists the program (MATH_CHECKS): the host-check test's build picks it up."""
    p = subprocess.run(["make", "-C", CSRC, "-n", "hostcheck", "-B"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "contact_cells_check_asan" in p.stdout and "contact_cells_check_tsan" in p.stdout
