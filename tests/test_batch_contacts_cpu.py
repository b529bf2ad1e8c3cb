"""sb_batch_contacts_device without a GPU: declared, exported, bound with its prototype, the NULL-handle error before a device is
looked for; tests/batch_contacts_ref.py against a scene worked out by hand; and the reference side of every case of
tests/test_gpu_batch_contacts.py, with the properties the GPU test relies on -- so that it cannot pass vacuously."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
import batch_grid_cases as gc  # noqa: E402
import batch_contacts_cases as cs  # noqa: E402
import batch_contacts_ref as cr  # noqa: E402

F = np.float32


def test_header_declares_and_library_exports_the_call(sb):
    names = sb.engine.declared_symbols()
    L = sb.batch.load_library()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert "sb_batch_contacts_device" in names and hasattr(L, "sb_batch_contacts_device")
    assert L.sb_batch_contacts_device.restype is ctypes.c_int and L.sb_batch_contacts_device.argtypes == [vp, u32, vp, vp, vp, u32, vp]
    assert L.sb_abi_version() == 1   # additions only
    header = open(sb.engine.HEADER_PATH).read()
    for needle in ("#define SB_BATCH_CONTACT_WORDS 4u", "#define SB_BATCH_CONTACTS_OTHER_BODY 1u", "#define SB_BATCH_WALL_LEFT 1u",
                   "#define SB_BATCH_WALL_RIGHT 2u", "#define SB_BATCH_WALL_LOW 4u", "#define SB_BATCH_WALL_HIGH 8u", "contact_words",
                   "contacts_kernel_vgprs", "contacts_kernel_scratch_bytes", "contacts_lds_bytes", "contacts_cells_per_side", "_contacts_device only ENQUEUE"):
        assert needle in header, needle


def test_python_has_the_call_and_the_constants(sb):
    b = sb.batch
    assert callable(sb.BatchEngine.contacts)
    assert b.CONTACT_WORDS == cr.WORDS == 4 == len(b.CONTACT_TOUCH_FIELDS) == len(b.CONTACT_COUNT_FIELDS)
    assert b.CONTACT_TOUCH_FIELDS == ("touching", "touching_other_body", "walls", "first_partner")
    assert b.CONTACT_COUNT_FIELDS == ("pairs", "other_body_pairs", "wall_particles", "touching_particles")
    assert (b.WALL_LEFT, b.WALL_RIGHT, b.WALL_LOW, b.WALL_HIGH) == (cr.LEFT, cr.RIGHT, cr.LOW, cr.HIGH) == (1, 2, 4, 8)
    assert b.CONTACTS_OTHER_BODY == 1


def test_a_null_handle_is_invalid_with_a_message(sb):
    L = sb.batch.load_library()
    word = (ctypes.c_int32 * 32)()
    p = ctypes.cast(word, ctypes.c_void_p)
    assert L.sb_batch_contacts_device(None, 0, None, None, None, 0, None) == 1
    assert L.sb_batch_contacts_device(None, 0, p, p, p, 4, p) == 1
    assert b"sb_batch_contacts_device: null batch" in L.sb_batch_last_error(None)


def test_python_refuses_what_is_not_a_buffer(sb):
    be = sb.BatchEngine.__new__(sb.BatchEngine)
    be._h, be.device, be.n_scenes, be.max_particles, be.max_beams, be._ext_stream = None, 0, 2, 16, 16, None
    import torch
    for call in (lambda: be.contacts(touch="no"), lambda: be.contacts(touch=torch.zeros((2, 16, 4), dtype=torch.int32)),
                 lambda: be.contacts(counts=torch.zeros((2, 4), dtype=torch.int32)), lambda: be.contacts(pairs=2.5),
                 lambda: be.contacts(pairs=True), lambda: be.contacts(pairs=-1), lambda: be.contacts(pairs=torch.zeros((2, 3, 2), dtype=torch.int32)),
                 lambda: be.contacts(labels=torch.zeros((2, 16), dtype=torch.int32))):
        with pytest.raises(ValueError):
            call()


def test_reference_on_a_scene_worked_out_by_hand(sb):
    """Capacity 8, radius 10, bounds 100.  Slots hold data indices 6, 1, 4, 3, 7: 6 and 1 on one spot on the left wall, 4 at
    distance 12 from both, 3 at exactly 20 from 4 (no contact), 7 alone in the top right corner."""
    pts = np.zeros((5, 6), "f4")
    pts[:, :2] = [(10.0, 50.0), (10.0, 50.0), (22.0, 50.0), (42.0, 50.0), (95.0, 90.0)]
    buf = gc.free_particles(sb, 2, (8, 0), pts, [6, 1, 4, 3, 7])
    touch, pairs, counts = cr.contacts_ref(buf, 10.0, 100.0, max_pairs=4)
    assert touch.dtype == pairs.dtype == counts.dtype == np.int32
    none = [0, -1, 0, -1]
    assert touch.tolist() == [none, [2, -1, 1, 4], none, [0, -1, 0, -1], [2, -1, 0, 1], none, [2, -1, 1, 1], [0, -1, 10, -1]]
    assert pairs.tolist() == [[1, 4], [1, 6], [4, 6], [-1, -1]] and counts.tolist() == [3, -1, 3, 3]
    labels = np.array([-1, 1, -1, 3, 1, -1, 6, 7], np.int32)           # 1 and 4 are one body
    touch, pairs, counts = cr.contacts_ref(buf, 10.0, 100.0, labels=labels, max_pairs=1, other_body=True)
    assert touch[:, 1].tolist() == [0, 1, 0, 0, 1, 0, 2, 0] and counts.tolist() == [3, 2, 3, 3] and pairs.tolist() == [[1, 6]]
    assert cr.contacts_ref(buf, 10.0, 100.0, labels=labels, max_pairs=3, other_body=True)[1].tolist() == [[1, 6], [4, 6], [-1, -1]]
    assert cr.contacts_ref(buf, 10.0, 100.0, max_pairs=2)[1].tolist() == [[1, 4], [1, 6]]
    buf.particle_count = 0
    assert [x.tolist() for x in cr.contacts_ref(buf, 10.0, 100.0, max_pairs=2)] == [x.tolist() for x in cr.never_uploaded(8, 2)]
    assert cr.never_uploaded(2, 1, True)[0].tolist() == [[0, 0, 0, -1]] * 2 and cr.never_uploaded(2, 1, True)[2].tolist() == [0, 0, 0, 0]
    assert cr.never_uploaded(2, 1)[2].tolist() == [0, -1, 0, 0]


@pytest.fixture(scope="module")
def expected(sb, oracle):
    """Every case on one oracle per scene, once: {name: (case, {op index: (touch, pairs, counts, labels)})}."""
    return {c["name"]: (c, cs.expected_contacts(oracle, c)) for c in cs.all_cases(sb)}


def test_every_case_runs_and_its_pair_list_holds_every_pair(expected):
    """max_pairs of every case is large enough at every point of its program; the lists are strictly ascending, the tails -1; the
    relation is symmetric: the per-particle counts sum to twice the pair counts."""
    assert len(expected) == 21
    for name, (case, exp) in expected.items():
        n, maxP, M = len(case["bufs"]), case["cap"][0], case["max_pairs"]
        assert sorted(exp) == list(range(-1, len(case["program"]))), name
        for k, (touch, pairs, counts, labels) in exp.items():
            assert touch.shape == (n, maxP, 4) and pairs.shape == (n, M, 2) and counts.shape == (n, 4), name
            assert touch.dtype == pairs.dtype == counts.dtype == np.int32, name
            for i in range(n):
                c = int(counts[i, 0])
                assert c <= M, (name, k, i, c)
                rows = [tuple(r) for r in pairs[i, :c].tolist()]
                assert all(a < b for a, b in zip(rows, rows[1:])) and all(r[0] < r[1] for r in rows), (name, k, i)
                assert (pairs[i, c:] == -1).all(), (name, k, i)
                assert touch[i, :, 0].sum() == 2 * c and touch[i, :, 1].sum() == 2 * counts[i, 1], (name, k, i)
                assert counts[i, 2] == (touch[i, :, 2] != 0).sum() and counts[i, 3] == (touch[i, :, 0] > 0).sum(), (name, k, i)
                assert ((touch[i, :, 3] >= 0) == (touch[i, :, 0] > 0)).all(), (name, k, i)
                live = labels[i] >= 0
                assert not touch[i, ~live, 0].any() and (touch[i, ~live, 3] == -1).all() and not touch[i, ~live, 2].any(), (name, k, i)


def test_every_wall_bit_occurs_exactly_where_it_should(sb, expected):
    case, exp = expected["on the walls"]
    buf = case["bufs"][0]
    touch = exp[-1][0][0]
    idx = buf.mapping[:buf.particle_count].astype(np.int64)
    want = [w for _, _, w in cs.wall_points()]
    assert touch[idx, 2].tolist() == want and sorted(set(want)) == [0, cr.LEFT, cr.RIGHT, cr.LOW, cr.HIGH]
    assert want.count(0) == 4 and exp[-1][2][0].tolist() == [0, 0, 8, 0]
    # the step clamps what was outside onto lo / hi exactly
    after = exp[0][0][0]
    assert (after[idx[[0, 1]], 2] == [cr.LEFT, cr.LOW]).all()
    # the pile lies in the corner of the floor and the left wall; a corner particle carries two bits
    assert {1, 4} <= set(np.unique(expected["pile"][1][1][0][0, :, 2]).tolist())
    one = expected["never uploaded, empty, one particle"][1][-1]
    assert one[0][2, 5].tolist() == [0, 0, cr.LEFT | cr.HIGH, -1] and one[2].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]
    assert (one[0][0] == [0, 0, 0, -1]).all() and (one[0][1] == [0, 0, 0, -1]).all()


def test_a_pair_at_distance_zero_occurs(sb, expected):
    case, exp = expected["permuted mapping + coincident particles"]
    buf = case["bufs"][1]
    touch, pairs, counts, labels = exp[-1]
    assert counts[1].tolist() == [4, 4, 0, 5]                         # two on one spot, three on another: 1 + 3 pairs
    assert [tuple(p) for p in pairs[1, :4].tolist()] == [(3, 40), (5, 17), (5, 29), (17, 29)]
    assert (buf.particles[3, :2] == buf.particles[40, :2]).all() and touch[1, 40].tolist() == [1, 1, 0, 3]
    spot = cs.case_edges(sb)["bufs"][0]
    assert max(t[0] for t in expected["cell edges"][1][-1][0][0].tolist()) >= 5      # six on one spot


def find(buf, x, y):
    d = np.nonzero((buf.particles[:, 0] == F(x)) & (buf.particles[:, 1] == F(y)))[0]
    assert len(d) == 1
    return int(d[0])


def test_the_pair_at_exactly_2r_is_absent_and_the_one_an_ulp_closer_present_across_a_cell_border(sb, expected):
    case, exp = expected["cell edges"]
    buf = case["bufs"][0]
    pairs = {tuple(p) for p in exp[-1][1][0].tolist()}
    g, cell = gc.cell_geometry(1000.0, 10.0, case["cap"][0])
    a0 = F(10) * cell - F(10.0)
    fars = (cs.dn(a0 + F(20.0)), a0 + F(20.0), cs.up(a0 + F(20.0)))
    assert int(a0 / cell) == 9 and all(int(f / cell) == 10 for f in fars)          # the border between cells 9 and 10
    for m, far in enumerate(fars):
        for a, b in ((find(buf, a0, 40.0 + 40.0 * m), find(buf, far, 40.0 + 40.0 * m)),      # across a border in x
                     (find(buf, 700.0 + 40.0 * m, a0), find(buf, 700.0 + 40.0 * m, far))):   # and in y
            assert ((min(a, b), max(a, b)) in pairs) == (m == 0), (m, a, b)


def test_nan_and_infinite_particles_touch_nothing(sb, expected):
    case, exp = expected["out of range"]
    buf = case["bufs"][0]
    assert not np.isfinite(buf.particles[12:15, :2]).all(axis=1).any()
    for k, (touch, pairs, counts, labels) in exp.items():
        assert not touch[0, 12:15, 0].any() and (touch[0, 12:15, 3] == -1).all(), k
        assert not np.isin(pairs[0], [12, 13, 14]).any(), k
    assert exp[-1][2][0, 0] == 17                                       # the dozen ordinary ones touch
    assert exp[-1][0][0, 12, 2] == 0 and exp[-1][0][0, 13, 2] == cr.RIGHT              # (NaN, 500): no bit; (+inf, 520): the right wall
    assert exp[-1][0][0, 14, 2] == cr.LEFT and exp[-1][0][0, 15, 2] == (cr.LEFT | cr.HIGH)    # (-inf, NaN); (-50, 1050)


def test_the_two_bodies_have_both_kinds_of_pair(sb, expected):
    case, exp = expected["two bodies that touch"]
    buf, D, body = cs.two_bodies(sb)
    touch, pairs, counts, labels = exp[-1]
    assert counts[0].tolist() == [22, 3, 0, 15] and counts[1].tolist() == [0, 0, 0, 0]
    assert len(set(labels[0, D[body == 0]].tolist())) == 1 and len(set(labels[0, D].tolist())) == 2
    cross = cr.contacts_ref(buf, labels=labels[0], max_pairs=8, other_body=True)[1]
    listed = [tuple(p) for p in cross[:3].tolist()]
    assert (cross[3:] == -1).all() and listed == sorted(listed) and all(labels[0, i] != labels[0, j] for i, j in listed)
    every = [tuple(p) for p in pairs[0, :22].tolist()]
    assert listed == [p for p in every if labels[0, p[0]] != labels[0, p[1]]] and listed != every[:3]


def test_the_pile_has_more_pairs_than_the_truncations(sb, expected):
    case, exp = expected["pile"]
    for k in exp:
        assert exp[k][2][0, 0] > max(cs.TRUNCATIONS) + 1, k
    assert exp[-1][2][0, 0] == len(cr.all_pairs(case["bufs"][0]))


def test_the_geometries_bite(sb, expected):
    assert expected["geometry 1000 / 600"][1][-1][2][0, 0] == 144 * 143 // 2           # one cell: every pair
    assert expected["geometry 100 / 10"][1][1][2][0, 0] > 1000                          # squeezed into the box
    assert max(int(e[2][:, 0].max()) for e in expected["heterogeneous"][1].values()) > 500
    assert gc.cell_geometry(1000.0, 10.0, 1024)[0] == 49 and gc.cell_geometry(1000.0, 600.0, 1024)[0] == 1
