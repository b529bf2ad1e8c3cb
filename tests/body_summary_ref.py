"""The rows, exact counts and ranks of sb_body_summary_device (include/softbody.h), restated in numpy the dense
way: per group a masked tree of W float64 leaves (leaf i = the value at DATA index i if particle i is finite and in the group, else
+0.0) reduced by tests/batch_summary_ref.py's tree_sum, a zero sum +0.0; int64 counts; extremes by the ORDERED KEYS of the floats
(-0.0 below +0.0; tests/float_keys.py).  On a scene that also fits a batch it gives tests/batch_body_summary_ref.py's rows, bit
for bit.  Only the rows that are asked for are summed, so a scene of thousands of groups costs max_rows trees.

A group of at most two members needs no tree (direct=True, the default): by the pin's own rules a lone leaf among +0.0s comes out
as itself (-0.0 as +0.0), and two leaves meet in exactly ONE addition of the tree -- each of them x + 0.0 + .. = x before it -- and
IEEE addition commutes, so the sum is (a + b) + 0.0 whatever W and the two data indices are.  direct_rows() takes all such rows
at once, which is what makes a scene of 262 000 pairs and single particles affordable; larger groups keep the dense tree.
tests/test_body_summary_cpu.py asserts direct=True against direct=False bit for bit."""
import numpy as np

import batch_body_summary_ref as qr
import batch_summary_ref as sr
from float_keys import fkey, key_max, key_min, unkey  # noqa: F401 (the ordered keys, -0.0 below +0.0)

WORDS, COUNT_WORDS = 24, 8
QNAN = sr.QNAN
SUMMARY_SHARED_WORDS = qr.SUMMARY_SHARED_WORDS
EMPTY_COUNTS = (0, 0, -1, 0, 0, 0, 0, 0)


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


def direct_rows(buf, grp, names, sizes, ks, gs, of, live, flagged, rows, counts):
    """rows[ks] / counts[ks] of the groups gs, each of one or two members, all at once.  names / sizes: every group of the scene,
    ascending, and its particles; of: the group of every live beam (-1: none)."""
    present = np.nonzero(grp >= 0)[0]
    by_group = present[np.argsort(grp[present], kind="stable")]             # members, group ascending, data index ascending
    first = (np.cumsum(sizes) - sizes)[np.searchsorted(names, gs)]
    two = sizes[np.searchsorted(names, gs)] == 2
    m = np.stack([by_group[first], by_group[np.where(two, first + 1, first)]])      # [2, n] data indices (a single one twice)
    n = len(gs)
    with np.errstate(all="ignore"):
        rec = buf.particles[m]                                                  # [2, n, 6]
        fin = np.isfinite(rec).all(axis=2)
        fin[1] &= two
        leaf = np.stack([np.where(fin[k], qr.leaves_of(rec[k]), 0.0) for k in range(2)])    # [2, 6, n]; +0.0 for what is not finite
        sums = (leaf[0] + leaf[1]) + 0.0
        nfin = fin.sum(axis=0)
        # beams: per group by its place in gs (beams of other groups fall out)
        place = np.full(len(names), -1, np.int64)
        place[np.searchsorted(names, gs)] = np.arange(n)
        mine = of >= 0
        at = np.full(len(of), -1, np.int64)
        at[mine] = place[np.searchsorted(names, of[mine])]
        mine = at >= 0
        strain, stress = buf.beams["strain"][live], buf.beams["stress"][live]
        bfin = np.isfinite(strain) & np.isfinite(stress)
        nbeam = np.bincount(at[mine], minlength=n)
        nbfin = np.bincount(at[mine & bfin], minlength=n)
        npend = np.bincount(at[mine & flagged], minlength=n)
        kmax_strain, kmax_stress, kmin_stress = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.full(n, 0xFFFFFFFF, np.uint32)
        ok = mine & bfin
        np.maximum.at(kmax_strain, at[ok], fkey(strain[ok]))
        np.maximum.at(kmax_stress, at[ok], fkey(stress[ok]))
        np.minimum.at(kmin_stress, at[ok], fkey(stress[ok]))
        members = np.where(two, 2, 1)
        counts[ks] = np.stack([members, nbeam, gs, npend, members - nfin, nbeam - nbfin, nfin, np.zeros(n, np.int64)], axis=1)
        out = np.repeat(qr.empty_row()[None, :], n, axis=0)
        out[:, :6] = counts[ks, :6].astype(np.float32)
        some = nfin > 0
        for c in range(4):
            out[some, 6 + c] = (sums[c][some] / nfin[some].astype(np.float64)).astype(np.float32)
        big, small = np.uint32(0xFFFFFFFF), np.uint32(0)
        for w, col, low in ((10, 0, True), (11, 1, True), (12, 0, False), (13, 1, False)):
            k = np.where(fin, fkey(rec[:, :, col]), big if low else small)
            out[some, w] = unkey(k.min(axis=0) if low else k.max(axis=0))[some]
        f = rec.astype(np.float64)
        v2 = np.where(fin, f[:, :, 2] * f[:, :, 2] + f[:, :, 3] * f[:, :, 3], -1.0).max(axis=0)
        out[some, 15] = v2[some].astype(np.float32)
        out[:, 14], out[:, 19] = sums[4].astype(np.float32), sums[5].astype(np.float32)
        has = nbfin > 0
        out[has, 16], out[has, 17], out[has, 18] = unkey(kmax_strain)[has], unkey(kmax_stress)[has], unkey(kmin_stress)[has]
    rows[ks] = out


def body_summary_ref(buf, labels, max_rows, pending_slots=None, direct=True):
    """(rows [max_rows, 24] float32, counts [max_rows, 8] int64, rank [maxP] int32).  buf: the scene now, a layout.Buffers as
    OracleEngine.load_buffers returns it; labels [maxP] integers at data indices; pending_slots: per beam slot "its break flag is
    set" (None: none is); direct: rows of groups of at most two members without a tree (False: every row by its dense trees)."""
    maxP, Bc = buf.max_particles, buf.beam_count
    assert 1 <= max_rows <= maxP
    grp = groups_of(buf, labels)
    rows = np.repeat(qr.empty_row()[None, :], max_rows, axis=0)
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
    shown = order[:max_rows]
    small = (sizes[shown] <= 2) if direct else np.zeros(len(shown), bool)
    if small.any():
        direct_rows(buf, grp, names, sizes, np.nonzero(small)[0], names[shown[small]], of, live, flagged, rows, counts)
    with np.errstate(all="ignore"):   # (non-finite state is data here; a sum beyond float32 becomes +inf on purpose)
        for k in np.nonzero(~small)[0]:
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
