"""The summary row of sb_batch_summary_device (include/softbody.h), restated in numpy: the reference of
tests/test_gpu_batch_summary.py and, on the oracle alone, of tests/test_batch_summary_cpu.py.

The sums are the pinned ones: float64, leaf i = the value at DATA index i (+0.0 where no finite particle / beam lives),
i = 0 .. W-1 with W the smallest power of two >= the capacity, reduced by the stride-halving tree.  The extremes are taken in the
order of the floats' keys: -0.0 below +0.0 (tests/float_keys.py)."""
import numpy as np

from float_keys import key_max, key_min

WORDS = 24
QNAN = np.uint32(0x7FC00000).view(np.float32)


def pow2_at_least(n):
    w = 1
    while w < n:
        w *= 2
    return w


def tree_sum(leaves):
    """for h = W/2, W/4, .. 1: s[i] += s[i + h] (i < h), in float64."""
    s = np.asarray(leaves, dtype=np.float64)
    assert len(s) == pow2_at_least(len(s))
    while len(s) > 1:
        h = len(s) // 2
        s = s[:h] + s[h:]
    return s[0]


def popcount(words):
    return int(sum(bin(int(w)).count("1") for w in np.asarray(words).ravel()))


def pending_of(ref):
    """The bits set in an OracleEngine's delete mask: break flags that wait for the next delete pass."""
    return popcount(ref.delete)


def never_uploaded_row():
    row = np.full(WORDS, QNAN, dtype=np.float32)
    row[[0, 1, 2, 3, 4, 5, 14, 20, 21, 22, 23]] = 0.0
    return row


def summary_ref(buf, uploaded_exists, pending):
    """One row.  buf: the scene now, a layout.Buffers as load_scene / OracleEngine.load_buffers return it; uploaded_exists: the
    Buffers that were uploaded (which data indices hold a particle / a beam, so which beams have been removed since);
    pending: the number of break flags set among the live beam slots."""
    up = uploaded_exists
    maxP, maxB = buf.max_particles, buf.max_beams
    P, Bc = buf.particle_count, buf.beam_count
    pidx = up.mapping[:up.particle_count].astype(np.int64)
    bidx0 = up.mapping[maxP:maxP + up.beam_count].astype(np.int64)
    live = buf.mapping[maxP:maxP + Bc].astype(np.int64)
    removed = np.setdiff1d(bidx0, live)
    row = np.zeros(WORDS, dtype=np.float32)
    with np.errstate(all="ignore"):   # (non-finite state is data here; a sum beyond float32 becomes +inf on purpose)
        Wp, Wb = pow2_at_least(maxP), pow2_at_least(maxB)
        leaf = np.zeros((5, Wp), dtype=np.float64)
        rec = buf.particles[pidx]
        fin = np.isfinite(rec).all(axis=1) if len(pidx) else np.zeros(0, bool)
        f = rec[fin].astype(np.float64)
        v2 = f[:, 2] * f[:, 2] + f[:, 3] * f[:, 3]
        d = pidx[fin]
        leaf[0, d], leaf[1, d], leaf[2, d], leaf[3, d], leaf[4, d] = f[:, 0], f[:, 1], f[:, 2], f[:, 3], 0.5 * v2
        n = int(fin.sum())
        row[0], row[1], row[2], row[3] = P, Bc, len(removed), pending
        row[4] = len(pidx) - n
        row[6:14] = QNAN
        row[15] = QNAN
        if n:
            for k in range(4):
                row[6 + k] = np.float32(tree_sum(leaf[k]) / np.float64(n))
            row[10], row[11] = key_min(rec[fin][:, 0]), key_min(rec[fin][:, 1])
            row[12], row[13] = key_max(rec[fin][:, 0]), key_max(rec[fin][:, 1])
            row[15] = np.float32(v2.max())
        row[14] = np.float32(tree_sum(leaf[4]))
        strain, stress = buf.beams["strain"][live], buf.beams["stress"][live]
        bfin = np.isfinite(strain) & np.isfinite(stress)
        nb = int(bfin.sum())
        row[5] = len(live) - nb
        row[16:20] = QNAN
        if nb:
            bl = np.zeros(Wb, dtype=np.float64)
            bl[live[bfin]] = strain[bfin].astype(np.float64)
            row[16], row[17], row[18] = key_max(strain[bfin]), key_max(stress[bfin]), key_min(stress[bfin])
            row[19] = np.float32(tree_sum(bl) / np.float64(nb))
        row[20] = 1.0
    return row


def rows_of(refs, bufs):
    """The [n, 24] table of one oracle per scene (None: never uploaded), as the batch's summary() returns it."""
    out = []
    for ref, buf in zip(refs, bufs):
        out.append(never_uploaded_row() if ref is None else summary_ref(ref.load_buffers(buf.copy()), buf, pending_of(ref)))
    return np.stack(out)


def assert_rows_equal(got, exp, what=""):
    """Every word by its bits -- sums, means, counts and extremes (a zero extreme has the sign the keys' order gives it); NaN words
    as `is NaN`."""
    got, exp = np.asarray(got, dtype=np.float32), np.asarray(exp, dtype=np.float32)
    assert got.shape == exp.shape and got.shape[-1] == WORDS, (what, got.shape, exp.shape)
    g2, e2 = got.reshape(-1, WORDS), exp.reshape(-1, WORDS)
    for r in range(len(g2)):
        for w in range(WORDS):
            g, e = g2[r, w], e2[r, w]
            where = "%s: row %d word %d: got %r, expected %r" % (what, r, w, g, e)
            if np.isnan(e):
                assert np.isnan(g), where
            else:
                assert g.view(np.uint32) == e.view(np.uint32), where
