"""The rows and ranks of sb_batch_body_summary_device (include/softbody.h), restated in numpy: the reference of
tests/test_gpu_batch_body_summary.py and, on the oracle alone, of tests/test_batch_body_summary_cpu.py.

The sums are the pinned ones, built the dense and obviously right way: per group a masked tree of W float64 leaves (leaf i = the
value at DATA index i if particle i is finite and in the group, else +0.0) reduced by tests/batch_summary_ref.py's tree_sum; a
sum that is zero is +0.0.  replay_route() is the other way round: the kernel's sparse route, step by step, for the CPU test that
shows both give the same bits."""
import numpy as np

import batch_bodies_ref as br
import batch_summary_ref as sr
from float_keys import key_max, key_min

WORDS = 24
QNAN = sr.QNAN
COUNT_WORDS, SUM_WORDS, EXTREME_WORDS = (0, 1, 2, 3, 4, 5, 20, 21, 22, 23), (6, 7, 8, 9, 14, 19), (10, 11, 12, 13, 15, 16, 17, 18)
SUMMARY_SHARED_WORDS = (0, 1) + tuple(range(3, 19))   # of a one-body scene's row 0: equal to summary()'s words
INT32_MIN = -2 ** 31


def empty_row():
    row = np.full(WORDS, QNAN, dtype=np.float32)
    row[[0, 1, 3, 4, 5, 14, 19, 20, 21, 22, 23]] = 0.0
    row[2] = -1.0
    return row


def never_uploaded(max_particles, max_rows):
    """(rows, rank) of a scene never uploaded -- and of one without particles."""
    return np.stack([empty_row()] * max_rows), np.full(max_particles, -1, np.int32)


def groups_of(buf, labels):
    """grp [maxP] int64: the group of the particle at every data index, -1 where there is no particle or no group.  Labels at
    data indices that hold no particle are never looked at."""
    maxP = buf.max_particles
    grp = np.full(maxP, -1, np.int64)
    for d in buf.mapping[:buf.particle_count].astype(np.int64):
        g = int(labels[d])
        if 0 <= g < maxP:
            grp[d] = g
    return grp


def leaves_of(rec):
    """The six float64 leaves of finite particle records [n, 6]: x, y, vx, vy, 0.5 (vx^2 + vy^2), x vy - y vx."""
    f = rec.astype(np.float64)
    x, y, vx, vy = f[:, 0], f[:, 1], f[:, 2], f[:, 3]
    return np.stack([x, y, vx, vy, 0.5 * (vx * vx + vy * vy), x * vy - y * vx])


def pending_slots_of(ref, buf):
    """Per beam slot of an OracleEngine (whose Buffers have buf's capacity): its break flag waits for the next delete pass."""
    bits = np.unpackbits(ref.delete.view(np.uint8), bitorder="little")
    return bits[buf.max_particles:buf.max_particles + buf.max_beams].astype(bool)


def body_summary_ref(buf, labels, max_rows, pending_slots=None):
    """(rows [max_rows, 24] float32, rank [maxP] int32) of one scene.  buf: the scene now, a layout.Buffers as load_scene /
    OracleEngine.load_buffers return it; labels [maxP] integers at data indices; pending_slots: per beam slot "its break flag
    is set" (None: none is)."""
    maxP, Bc = buf.max_particles, buf.beam_count
    assert 1 <= max_rows <= maxP
    W = sr.pow2_at_least(maxP)
    grp = groups_of(buf, labels)
    rows, rank = never_uploaded(maxP, max_rows)
    present = np.nonzero(grp >= 0)[0]
    names = sorted(set(grp[present].tolist()))
    sizes = {g: int((grp == g).sum()) for g in names}
    order = sorted(names, key=lambda g: (-sizes[g], g))
    live = buf.mapping[maxP:maxP + Bc].astype(np.int64)
    ga, gb = grp[buf.beams["a"][live].astype(np.int64)], grp[buf.beams["b"][live].astype(np.int64)]
    flagged = np.zeros(Bc, bool) if pending_slots is None else np.asarray(pending_slots[:Bc], bool)
    with np.errstate(all="ignore"):   # (non-finite state is data here; a sum beyond float32 becomes +inf on purpose)
        finite = np.isfinite(buf.particles).all(axis=1)
        for k, g in enumerate(order):
            rank[grp == g] = k
            if k >= max_rows:
                continue
            row = rows[k]
            members = np.nonzero(grp == g)[0]
            fin = members[finite[members]]
            mine = (ga == g) & (gb == g)
            strain, stress = buf.beams["strain"][live[mine]], buf.beams["stress"][live[mine]]
            bfin = np.isfinite(strain) & np.isfinite(stress)
            row[0], row[1], row[2], row[3] = len(members), int(mine.sum()), g, int((flagged & mine).sum())
            row[4], row[5] = len(members) - len(fin), int(mine.sum()) - int(bfin.sum())
            leaf = np.zeros((6, W), dtype=np.float64)
            leaf[:, fin] = leaves_of(buf.particles[fin])
            sums = [sr.tree_sum(leaf[c]) + 0.0 for c in range(6)]   # (+ 0.0: a zero sum is +0.0)
            if len(fin):
                rec = buf.particles[fin]
                for c in range(4):
                    row[6 + c] = np.float32(sums[c] / np.float64(len(fin)))
                # (extremes in the order of the keys: -0.0 below +0.0)
                row[10], row[11], row[12], row[13] = key_min(rec[:, 0]), key_min(rec[:, 1]), key_max(rec[:, 0]), key_max(rec[:, 1])
                f = rec.astype(np.float64)
                row[15] = np.float32((f[:, 2] * f[:, 2] + f[:, 3] * f[:, 3]).max())
            row[14], row[19] = np.float32(sums[4]), np.float32(sums[5])
            if bfin.any():
                row[16], row[17], row[18] = key_max(strain[bfin]), key_max(stress[bfin]), key_min(stress[bfin])
    return rows, rank


def body_summary_of(bufs_now, labels, max_rows, pending=None):
    """(rows [n, max_rows, 24], rank [n, maxP]) of a batch from one Buffers per scene (None: never uploaded), labels [n, maxP] and
    (optionally) one pending-slot array per scene."""
    maxP = labels.shape[1]
    out = [never_uploaded(maxP, max_rows) if b is None else body_summary_ref(b, labels[i], max_rows, None if pending is None else pending[i])
           for i, b in enumerate(bufs_now)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def body_labels_of(bufs_now, max_particles):
    """bodies()' labels [n, maxP] of a batch from one Buffers per scene (None: never uploaded)."""
    return br.bodies_of(bufs_now, max_particles)[0]


def assert_rows_equal(got, exp, what=""):
    """Every word by its bits: counts, the label, sums, means and extremes; NaN words as `is NaN`."""
    got, exp = np.asarray(got, dtype=np.float32), np.asarray(exp, dtype=np.float32)
    assert got.shape == exp.shape and got.shape[-1] == WORDS, (what, got.shape, exp.shape)
    g2, e2 = got.reshape(-1, WORDS), exp.reshape(-1, WORDS)
    same = (g2.view(np.uint32) == e2.view(np.uint32)) | (np.isnan(g2) & np.isnan(e2))
    for r, w in zip(*np.nonzero(~same)):
        assert False, "%s: row %d word %d: got %r, expected %r" % (what, r, w, g2[r, w], e2[r, w])


def assert_equal(got, exp, what=""):
    """(rows, rank) against (rows, rank)."""
    assert_rows_equal(got[0], exp[0], what)
    g, e = np.asarray(got[1]), np.asarray(exp[1])
    assert g.dtype == np.int32 and g.shape == e.shape, (what, g.dtype, g.shape, e.shape)
    if not np.array_equal(g, e):
        at = tuple(int(x[0]) for x in np.nonzero(g != e))
        raise AssertionError("%s: ranks differ in %d words, first at %s: got %d, expected %d" % (what, int((g != e).sum()), at, g[at], e[at]))


# ---------------------------------------------------------------- the kernel's route, one step at a time
def bitrev(i, bits):
    r = 0
    for k in range(bits):
        r |= ((i >> k) & 1) << (bits - 1 - k)
    return r


def replay_route(grp, member, leaves, W):
    """{group: float64 sum} of one column the way k_batch_body_summary takes: the members (member[i]: particle i is finite and in
    group grp[i]; leaves[i] its leaf) sorted by the key grp * W + bitrev(i), then log2 W levels in which a block's head adds its
    partial sum onto the head of its left sibling block.  Every addition is one float64 addition; nothing is masked."""
    bits = W.bit_length() - 1
    assert 1 << bits == W
    idx = [i for i in range(len(grp)) if member[i]]
    keyed = sorted((int(grp[i]) * W + bitrev(i, bits), i) for i in idx)
    keys = [k for k, _ in keyed]
    assert len(set(keys)) == len(keys)
    col = [np.float64(leaves[i]) for _, i in keyed]
    for l in range(bits):
        adds = []
        for q in range(1, len(keys)):
            key, prev = keys[q], keys[q - 1]
            if prev >> l == key >> l or not (key >> l) & 1 or prev >> (l + 1) != key >> (l + 1):
                continue
            want = ((key >> l) - 1) << l
            lo = min(p for p in range(q) if keys[p] >= want)   # (the lower bound)
            adds.append((lo, q))
        touched = [p for pair in adds for p in pair]
        assert len(set(touched)) == len(touched), "an operand is touched twice at level %d" % l
        for lo, q in adds:
            col[lo] = col[lo] + col[q]
    out = {}
    for q, key in enumerate(keys):
        if q == 0 or keys[q - 1] >> bits != key >> bits:
            out[key >> bits] = col[q] + 0.0
    return out
