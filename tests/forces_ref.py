"""The outputs of sb_forces_device (include/softbody.h) restated in plain numpy float32: tests/batch_forces_ref.py's
forces_ref on one scene with int64 counts.  A scene is a layout.Buffers as Engine.load_buffers / OracleEngine.load_buffers return it
at the call's place in the stream.  The engine's live-beam rule is that read-back's: the beam slots 0 .. beam_count - 1 of the mapping
are the caller slots of the latest upload that no delete pass has removed (the entries behind beam_count are stale after a
compaction), a beam with a pending break flag is still among them.  The partners of a particle are taken in ascending MAPPING-SLOT
order, the order of mapping[:particle_count].

The batch's three wrong variants pass through (descending, saturate, skip_slots); a fourth is the engine's own: by_data_index=True
takes the partners in ascending DATA-index order instead -- what a kernel that sorted sb_contacts_device's records would compute."""
import numpy as np

import batch_forces_ref as bfr

F = np.float32
WORDS, COUNT_WORDS, FIELDS = bfr.WORDS, bfr.COUNT_WORDS, bfr.FIELDS
words = bfr.words


def in_data_order(buf):
    """`buf` with its particle slots renumbered in ascending data-index order: the same scene by data index, another order of slots"""
    out = buf.copy()
    P = buf.particle_count
    out.mapping[:P] = np.sort(buf.mapping[:P])
    return out


def forces_ref(buf, radius=10.0, subticks=64, labels=None, other_body=False, by_data_index=False, **wrong):
    """(rows [maxP, 8] float32, beam_i32 [maxP, 2] int32, tension [maxB] float32, counts [4] int64)"""
    rows, beam_i32, tension, counts = bfr.forces_ref(in_data_order(buf) if by_data_index else buf, radius, subticks, labels, other_body, **wrong)
    return rows, beam_i32, tension, counts.astype(np.int64)


def assert_forces(got, exp, what):
    """every word of (rows, beam_i32, tension, counts); None in `got`: not asked for"""
    names = ("rows", "beam_i32", "tension", "counts")
    if got[3] is not None:
        g, e = [int(x) for x in np.asarray(got[3])], [int(x) for x in exp[3]]
        print(what, "counts", g, "expected", e)
        assert g == e, "%s: counts %s, expected %s" % (what, g, e)
    for name, g, e in zip(names[:3], got[:3], exp[:3]):
        if g is None:
            continue
        g = np.asarray(g)
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, g.dtype, e.shape, e.dtype)
        gw, ew = words(g).reshape(len(e), -1), words(e).reshape(len(e), -1)
        bad = np.flatnonzero((gw != ew).any(axis=1))
        assert bad.size == 0, "%s: %d %s rows differ, first %d: %s, expected %s" % (what, bad.size, name, bad[0], g[bad[0]], e[bad[0]])
