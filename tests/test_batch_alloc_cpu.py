"""csrc/sb_batch_alloc.h without a GPU: the free bitmap and the r-th free index of the batch's adding calls, built on the host
under sanitizers (tests/batch_alloc_check.cpp, `make hostcheck`), against numpy: the free indices are np.flatnonzero of the free
bytes.  Every capacity round the edges of a bitmap word, every occupancy pattern that puts the free indices at an edge, with one
and with two rows of bytes, in a scene never uploaded, and with garbage in the padding bytes past the capacity."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbody-webgpu_amd", "csrc")
CAPACITIES = (1, 31, 32, 33, 37, 61, 64, 65, 1024, 4096)


def patterns(cap, rng):
    """name -> occupancy bytes [cap] (nonzero: held)"""
    last_word = np.ones(cap, np.uint8)
    last_word[32 * ((cap - 1) // 32):] = 0
    only = lambda i: np.where(np.arange(cap) == i, 0, 1).astype(np.uint8)
    return {"all-free": np.zeros(cap, np.uint8), "none-free": np.full(cap, 1, np.uint8), "only-0": only(0), "only-last": only(cap - 1),
            "last-word": last_word, "alternating": (np.arange(cap) % 2).astype(np.uint8),
            "random": (rng.integers(0, 256, cap) * (rng.random(cap) < 0.6)).astype(np.uint8)}


def free_indices(cap, loaded, rows):
    """the three-line restatement"""
    held = np.zeros(cap, bool)
    for r in rows:
        held |= r[:cap] != 0
    return np.flatnonzero(~held) if loaded else np.zeros(0, np.int64)


def records():
    rng = np.random.default_rng(13)
    out = []
    for cap in CAPACITIES:
        pad = -cap % 4
        for name, occ in patterns(cap, rng).items():
            second = (rng.random(cap) < 0.3).astype(np.uint8) * 7          # a reset state that still owns some indices
            for rows in ([occ], [occ, second], [occ, np.zeros(cap, np.uint8)]):
                for loaded in (1, 0) if len(rows) == 1 else (1,):
                    for garbage in ((0,), (0xFF, 0)) if pad else ((0,),):
                        # (garbage: held-looking bytes must hide no index, free-looking bytes must not become one: both in one record,
                        # 0xFF in the first row's padding, 0 in the second's or, with one row, in a record of its own)
                        for g in garbage:
                            padded = [np.concatenate([r, np.full(pad, g if j == 0 else 0, np.uint8)]) for j, r in enumerate(rows)]
                            out.append((cap, loaded, padded, "%d %s rows=%d loaded=%d pad=%#x" % (cap, name, len(rows), loaded, g)))
    return out


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_header_equals_flatnonzero_under_sanitizers(tmp_path, san):
    exe = os.path.join(CSRC, "hostcheck_build", "batch_alloc_check_" + san)
    p = subprocess.run(["make", "-C", CSRC, os.path.join("hostcheck_build", "batch_alloc_check_" + san)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    recs = records()
    path = str(tmp_path / "records.bin")
    want = []
    with open(path, "wb") as f:
        for cap, loaded, rows, _ in recs:
            f.write(np.asarray([cap, loaded, len(rows)], "<u4").tobytes())
            for r in rows:
                assert len(r) % 4 == 0 and len(r) - cap < 4
                f.write(r.tobytes())
            free = free_indices(cap, loaded, rows)
            bits = np.zeros(32 * ((cap + 31) // 32), np.uint8)
            bits[free] = 1
            words = np.packbits(bits, bitorder="little").view("<u4")
            want.append(" ".join("%08x" % w for w in words) + " |" + "".join(" %d" % d for d in free))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, [(recs[i][3], got[i][:200], want[i][:200]) for i in bad[:5]]
    # the cases are what they are named for
    frees = {name: len(w.split("|")[1].split()) for (_, _, _, name), w in zip(recs, want)}
    assert frees["4096 all-free rows=1 loaded=1 pad=0x0"] == 4096 and frees["4096 all-free rows=1 loaded=0 pad=0x0"] == 0
    assert frees["37 only-last rows=1 loaded=1 pad=0xff"] == 1 and frees["37 none-free rows=1 loaded=1 pad=0x0"] == 0
    assert frees["65 last-word rows=1 loaded=1 pad=0xff"] == 1 and frees["1024 last-word rows=1 loaded=1 pad=0x0"] == 32
