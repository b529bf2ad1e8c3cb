"""The rows, moments and ranks of sb_batch_pose_device (include/softbody.h), restated in numpy: the reference of
tests/test_gpu_batch_pose.py and, on the oracle alone, of tests/test_batch_pose_cpu.py.

It does it the dense and obviously right way: per group and column a masked tree of W float64 leaves (leaf i = the value at DATA
index i if particle i is a matched member of the group, else +0.0) reduced by tests/batch_summary_ref.py's tree_sum, a sum that is
zero being +0.0; then the five expressions of the definition in np.float64.  Groups, labels and the ranking are
tests/batch_body_summary_ref.py's.  The reference configuration is always an array [maxP, 2] at data indices, NaN where a particle
has none: reference_of() makes the one that `ref = NULL` stands for from the scene's reset state."""
import numpy as np

import batch_body_summary_ref as qr
import batch_summary_ref as sr

WORDS, MOMENT_WORDS, NSUM = 24, 8, 11
QNAN = sr.QNAN
QNAN64 = np.uint64(0x7FF8000000000000).view(np.float64)
X, Y, RX, RY, VX, VY, D, C, Q, Q0, L = range(NSUM)


def empty_row():
    row = np.zeros(WORDS, dtype=np.float32)
    row[1] = -1.0
    row[4:17] = QNAN
    return row


def empty_moments():
    m = np.zeros(MOMENT_WORDS, dtype=np.float64)
    m[:5] = QNAN64
    return m


def never_uploaded(max_particles, max_rows):
    """(rows, moments, rank) of a scene never uploaded -- and of one without particles."""
    return np.stack([empty_row()] * max_rows), np.stack([empty_moments()] * max_rows), np.full(max_particles, -1, np.int32)


def reference_of(reset_buf):
    """The reference that `ref = NULL` stands for, from the scene's reset state (a layout.Buffers; None: never uploaded): x and y
    of the record at the data index of each of its particle slots, NaN at every other data index -- where a particle spawned
    since then lives."""
    if reset_buf is None:
        return None
    ref = np.full((reset_buf.max_particles, 2), np.nan, np.float32)
    d = reset_buf.mapping[:reset_buf.particle_count].astype(np.int64)
    ref[d] = reset_buf.particles[d, 0:2]
    return ref


def leaves_of(rec, ref):
    """The eleven float64 leaves [11, n] of matched particle records [n, 6] with references [n, 2]; every float cast to float64
    first, so each product is exact and each leaf is rounded once."""
    f, r = rec.astype(np.float64), ref.astype(np.float64)
    x, y, vx, vy, rx, ry = f[:, 0], f[:, 1], f[:, 2], f[:, 3], r[:, 0], r[:, 1]
    return np.stack([x, y, rx, ry, vx, vy, x * rx + y * ry, rx * y - ry * x, x * x + y * y, rx * rx + ry * ry, x * vy - y * vx])


def derive(S, n):
    """(a, b, I, I0, Lc) in np.float64 from the eleven sums and the matched count: exactly the definition's expressions."""
    S, n = [np.float64(s) for s in S], np.float64(n)
    a = S[D] - (S[X] * S[RX] + S[Y] * S[RY]) / n
    b = S[C] - (S[RX] * S[Y] - S[RY] * S[X]) / n
    i = S[Q] - (S[X] * S[X] + S[Y] * S[Y]) / n
    i0 = S[Q0] - (S[RX] * S[RX] + S[RY] * S[RY]) / n
    lc = S[L] - (S[X] * S[VY] - S[Y] * S[VX]) / n
    return a, b, i, i0, lc


def fill(row, mom, S, n):
    """Words 4 .. 16 of a row and the moments of a group of n >= 1 matched members with sums S."""
    n = np.float64(n)
    a, b, i, i0, lc = derive(S, n)
    for k in range(6):
        row[4 + k] = np.float32(np.float64(S[k]) / n)
    row[10], row[11], row[12], row[13], row[14] = (np.float32(v) for v in (a, b, i, i0, lc))
    row[15] = np.float32(lc / i) if i > 0 else QNAN
    row[16] = np.float32(i / i0) if i0 > 0 else QNAN
    mom[:] = [a, b, i, i0, lc, n, 0.0, 0.0]


def matched_of(buf, ref):
    """Per data index: the record there is finite and its reference is."""
    with np.errstate(all="ignore"):
        return np.isfinite(buf.particles).all(axis=1) & np.isfinite(np.asarray(ref, np.float32)).all(axis=1)


def pose_ref(buf, labels, max_rows, ref):
    """(rows [max_rows, 24] float32, moments [max_rows, 8] float64, rank [maxP] int32) of one scene.  buf: the scene now, a
    layout.Buffers; labels [maxP] integers at data indices; ref [maxP, 2] float32 at data indices, NaN where there is none."""
    maxP = buf.max_particles
    assert 1 <= max_rows <= maxP and np.asarray(ref).shape == (maxP, 2)
    W = sr.pow2_at_least(maxP)
    grp = qr.groups_of(buf, labels)
    rank = qr.body_summary_ref(buf, labels, 1)[1]          # (the ranking is the body summary's; it does not depend on max_rows)
    rows, moms, _ = never_uploaded(maxP, max_rows)
    ok = matched_of(buf, ref)
    ref = np.asarray(ref, np.float32)
    with np.errstate(all="ignore"):   # (a moment beyond float32 becomes inf on purpose)
        for k in range(min(max_rows, int(rank.max()) + 1)):
            members = np.nonzero(rank == k)[0]
            m = members[ok[members]]
            rows[k, 0], rows[k, 1], rows[k, 2], rows[k, 3] = len(members), grp[members[0]], len(m), len(members) - len(m)
            if len(m) == 0:
                continue
            leaf = np.zeros((NSUM, W), dtype=np.float64)
            leaf[:, m] = leaves_of(buf.particles[m], ref[m])
            fill(rows[k], moms[k], [sr.tree_sum(leaf[c]) + 0.0 for c in range(NSUM)], len(m))   # (+ 0.0: a zero sum is +0.0)
    return rows, moms, rank


def pose_of(bufs_now, labels, max_rows, refs):
    """(rows [n, max_rows, 24], moments [n, max_rows, 8], rank [n, maxP]) of a batch from one Buffers per scene (None: never
    uploaded), labels [n, maxP] and one reference array per scene."""
    maxP = labels.shape[1]
    out = [never_uploaded(maxP, max_rows) if b is None else pose_ref(b, labels[i], max_rows, refs[i]) for i, b in enumerate(bufs_now)]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def assert_equal(got, exp, what=""):
    """(rows, moments, rank) against (rows, moments, rank): every word by its bits, NaN words as `is NaN`, ranks exactly."""
    for name, g, e, dtype, bits in (("rows", got[0], exp[0], np.float32, np.uint32), ("moments", got[1], exp[1], np.float64, np.uint64)):
        if g is None:
            continue
        g, e = np.asarray(g), np.asarray(e)
        assert g.dtype == dtype and g.shape == e.shape, (what, name, g.dtype, g.shape, e.shape)
        same = (g.view(bits) == e.view(bits)) | (np.isnan(g) & np.isnan(e))
        if not same.all():
            at = tuple(int(x[0]) for x in np.nonzero(~same))
            raise AssertionError("%s: %s differ in %d words, first at %s: got %r, expected %r" % (what, name, int((~same).sum()), at, g[at], e[at]))
    if got[2] is not None:
        g, e = np.asarray(got[2]), np.asarray(exp[2])
        assert g.dtype == np.int32 and np.array_equal(g, e), (what, "rank")
