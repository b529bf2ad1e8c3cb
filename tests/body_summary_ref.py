"""The rows, exact counts and ranks of sb_body_summary_device (include/softbody.h), restated in numpy the dense
way: per group a masked tree of W float64 leaves (leaf i = the value at DATA index i if particle i is finite and in the group, else
+0.0) reduced by tests/batch_summary_ref.py's tree_sum, a zero sum +0.0; int64 counts; extremes by the ORDERED KEYS of the floats
(-0.0 below +0.0).  On a scene that also fits a batch it gives tests/batch_body_summary_ref.py's rows (that one compares floats:
its extremes agree by value).  Only the rows that are asked for are summed, so a scene of thousands of groups costs max_rows trees."""
import numpy as np

import batch_body_summary_ref as qr
import batch_summary_ref as sr

WORDS, COUNT_WORDS = 24, 8
QNAN = sr.QNAN
SUMMARY_SHARED_WORDS = qr.SUMMARY_SHARED_WORDS
EMPTY_COUNTS = (0, 0, -1, 0, 0, 0, 0, 0)


def fkey(x):
    """finite float32 values as uint32 keys of the same order, -0.0 below +0.0 (sbb_fkey)"""
    b = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def key_min(x):
    return unkey(fkey(x).min())


def key_max(x):
    return unkey(fkey(x).max())


def groups_of(buf, labels):
    """grp [maxP] int64: the group of the particle at every data index, -1 where there is no particle or no group.  Labels at
    data indices that hold no particle are never looked at."""
    maxP = buf.max_particles
    grp = np.full(maxP, -1, np.int64)
    pidx = buf.mapping[:buf.particle_count].astype(np.int64)
    lab = np.asarray(labels)[pidx].astype(np.int64)
    ok = (lab >= 0) & (lab < maxP)
    grp[pidx[ok]] = lab[ok]
    return grp


def group_sums(buf, grp, g, W=None):
    """The six pinned sums of group g and its finite members: masked trees of W leaves."""
    W = sr.pow2_at_least(buf.max_particles) if W is None else W
    members = np.nonzero(grp == g)[0]
    with np.errstate(all="ignore"):
        fin = members[np.isfinite(buf.particles[members]).all(axis=1)]
        leaf = np.zeros((6, W), dtype=np.float64)
        leaf[:, fin] = qr.leaves_of(buf.particles[fin])
        return [sr.tree_sum(leaf[c]) + 0.0 for c in range(6)], fin, members


def body_summary_ref(buf, labels, max_rows, pending_slots=None):
    """(rows [max_rows, 24] float32, counts [max_rows, 8] int64, rank [maxP] int32).  buf: the scene now, a layout.Buffers as
    OracleEngine.load_buffers returns it; labels [maxP] integers at data indices; pending_slots: per beam slot "its break flag is
    set" (None: none is)."""
    maxP, Bc = buf.max_particles, buf.beam_count
    assert 1 <= max_rows <= maxP
    grp = groups_of(buf, labels)
    rows = np.stack([qr.empty_row()] * max_rows)
    counts = np.tile(np.array(EMPTY_COUNTS, np.int64), (max_rows, 1))
    rank = np.full(maxP, -1, np.int32)
    present = np.nonzero(grp >= 0)[0]
    names, sizes = np.unique(grp[present], return_counts=True)
    order = np.lexsort((names, -sizes))
    rank_of = np.empty(len(names), np.int64)
    rank_of[order] = np.arange(len(names))
    rank[present] = rank_of[np.searchsorted(names, grp[present])]
    live = buf.mapping[maxP:maxP + Bc].astype(np.int64)
    ga, gb = grp[buf.beams["a"][live].astype(np.int64)], grp[buf.beams["b"][live].astype(np.int64)]
    of = np.where((ga == gb) & (ga >= 0), ga, -1)
    flagged = np.zeros(Bc, bool) if pending_slots is None else np.asarray(pending_slots[:Bc], bool)
    with np.errstate(all="ignore"):   # (non-finite state is data here; a sum beyond float32 becomes +inf on purpose)
        for k in range(min(max_rows, len(names))):
            g = int(names[order[k]])
            row = rows[k]
            sums, fin, members = group_sums(buf, grp, g)
            mine = of == g
            strain, stress = buf.beams["strain"][live[mine]], buf.beams["stress"][live[mine]]
            bfin = np.isfinite(strain) & np.isfinite(stress)
            counts[k] = (len(members), int(mine.sum()), g, int((flagged & mine).sum()), len(members) - len(fin),
                         int(mine.sum()) - int(bfin.sum()), len(fin), 0)
            row[:6] = counts[k, :6].astype(np.float32)
            if len(fin):
                rec = buf.particles[fin]
                for c in range(4):
                    row[6 + c] = np.float32(sums[c] / np.float64(len(fin)))
                row[10], row[11], row[12], row[13] = key_min(rec[:, 0]), key_min(rec[:, 1]), key_max(rec[:, 0]), key_max(rec[:, 1])
                f = rec.astype(np.float64)
                row[15] = np.float32((f[:, 2] * f[:, 2] + f[:, 3] * f[:, 3]).max())
            row[14], row[19] = np.float32(sums[4]), np.float32(sums[5])
            if bfin.any():
                row[16], row[17], row[18] = key_max(strain[bfin]), key_max(stress[bfin]), key_min(stress[bfin])
    return rows, counts, rank


def assert_equal(got, exp, what=""):
    """(rows, counts, rank) against (rows, counts, rank): every word by its bits (an entry of `got` may be None: not asked for)."""
    for name, g, e in zip(("rows", "counts", "rank"), got, exp):
        if g is None:
            continue
        g, e = np.ascontiguousarray(g), np.ascontiguousarray(e)
        assert g.dtype == e.dtype and g.shape == e.shape, (what, name, g.dtype, g.shape, e.dtype, e.shape)
        gb, eb = (g.view(np.uint32), e.view(np.uint32)) if name == "rows" else (g, e)
        if not np.array_equal(gb, eb):
            at = tuple(int(x[0]) for x in np.nonzero(gb != eb))
            raise AssertionError("%s: %s differ in %d words, first at %s: got %r, expected %r" % (what, name, int((gb != eb).sum()), at, g[at], e[at]))
