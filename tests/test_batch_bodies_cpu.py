"""sb_batch_bodies_device without a GPU: declared, exported, bound with its prototype, argument errors before a device is looked
for; tests/batch_bodies_ref.py against a scene worked out by hand; and the oracle side of every program of
tests/test_gpu_batch_bodies.py, with the figures the GPU test relies on (bodies that come apart, pending flags that still
connect, a delete pass that splits, stale mapping entries behind the live beam slots)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_bodies_cases as cs  # noqa: E402
import batch_bodies_ref as br  # noqa: E402
import batch_summary_ref as sr  # noqa: E402


def test_header_declares_and_library_exports_the_call(sb):
    names = sb.engine.declared_symbols()
    L = sb.batch.load_library()
    vp = ctypes.c_void_p
    assert "sb_batch_bodies_device" in names and hasattr(L, "sb_batch_bodies_device")
    assert L.sb_batch_bodies_device.restype is ctypes.c_int and L.sb_batch_bodies_device.argtypes == [vp, vp, vp, vp]
    assert L.sb_abi_version() == 1   # additions only
    header = open(sb.engine.HEADER_PATH).read()
    for needle in ("#define SB_BATCH_BODY_WORDS 4u", "body_words", "bodies_kernel_vgprs", "bodies_kernel_scratch_bytes"):
        assert needle in header, needle
    assert callable(sb.BatchEngine.bodies)


def test_a_null_handle_is_invalid_with_a_message(sb):
    L = sb.batch.load_library()
    word = (ctypes.c_int32 * 32)()
    p = ctypes.cast(word, ctypes.c_void_p)
    assert L.sb_batch_bodies_device(None, None, None, None) == 1
    assert L.sb_batch_bodies_device(None, p, p, p) == 1
    assert b"sb_batch_bodies_device" in L.sb_batch_last_error(None)


def test_body_fields_name_the_four_words(sb):
    f = sb.batch.BODY_FIELDS
    assert sb.batch.BODY_WORDS == br.WORDS == 4 == len(f)
    assert f == ("bodies", "largest_particles", "single_particles", "largest_label")
    assert "#define SB_BATCH_BODY_WORDS %du" % sb.batch.BODY_WORDS in open(sb.engine.HEADER_PATH).read()


def test_python_refuses_what_is_not_a_buffer(sb):
    be = sb.BatchEngine.__new__(sb.BatchEngine)
    be._h, be.device, be.n_scenes, be.max_particles, be.max_beams, be._ext_stream = None, 0, 2, 16, 16, None
    import torch
    for call in (lambda: be.bodies("no"), lambda: be.bodies(torch.zeros((2, 16), dtype=torch.int32)),
                 lambda: be.bodies(counts=torch.zeros((2, 4), dtype=torch.int32)), lambda: be.bodies(sizes=2.5)):
        with pytest.raises(ValueError):
            call()


def hand_scene(sb):
    """Capacity 12 / 8.  Particles at data indices 9, 2, 7, 4, 11, 5 (in that slot order); beams (data index: a - b)
    3: 9 - 7,  0: 7 - 4,  5: 4 - 9 (a triangle),  6: 11 - 2,  1: 2 - 11 (parallel);  5 is alone.  Beam slots: 3, 0, 5, 6, 1."""
    buf = sb.Buffers(2, 12, 8)
    idx = [9, 2, 7, 4, 11, 5]
    buf.mapping[:6] = idx
    for d in idx:
        buf.particles[d, :2] = (100.0 + 50.0 * d, 500.0)
    for slot, (d, a, b) in enumerate([(3, 9, 7), (0, 7, 4), (5, 4, 9), (6, 11, 2), (1, 2, 11)]):
        buf.beams[d]["a"], buf.beams[d]["b"], buf.beams[d]["length"] = a, b, 50.0
        buf.mapping[12 + slot] = d
    buf.particle_count, buf.beam_count = 6, 5
    return buf


def test_reference_on_a_scene_worked_out_by_hand(sb):
    buf = hand_scene(sb)
    labels, sizes, counts = br.bodies_ref(buf)
    assert labels.dtype == sizes.dtype == counts.dtype == np.int32
    assert labels.tolist() == [-1, -1, 2, -1, 4, 5, -1, 4, -1, 4, -1, 2]
    exp = np.zeros((12, 2), np.int32)
    exp[4], exp[2], exp[5] = (3, 3), (2, 2), (1, 0)
    assert np.array_equal(sizes, exp)
    assert counts.tolist() == [3, 3, 1, 4]
    # the delete pass removed beam 0 (7 - 4) and beam 6: the mapping's head is compacted, its tail keeps stale entries
    now = buf.copy()
    now.mapping[12:15] = (3, 5, 1)
    now.beam_count = 3
    assert now.mapping[15:17].tolist() == [6, 1]                      # stale: never edges
    labels, sizes, counts = br.bodies_ref(now)
    assert labels.tolist() == [-1, -1, 2, -1, 4, 5, -1, 4, -1, 4, -1, 2] and sizes[4].tolist() == [3, 2] and sizes[2].tolist() == [2, 1]
    now.mapping[12:14] = (3, 1)                                       # and beam 5 (4 - 9): particle 4 is on its own
    now.beam_count = 2
    labels, sizes, counts = br.bodies_ref(now)
    assert labels.tolist() == [-1, -1, 2, -1, 4, 5, -1, 7, -1, 7, -1, 2]
    assert counts.tolist() == [4, 2, 2, 2]                            # two bodies of 2: the smaller label wins
    # no beams, no particles, never uploaded
    now.beam_count = 0
    assert br.bodies_ref(now)[2].tolist() == [6, 1, 6, 2]
    now.particle_count = 0
    labels, sizes, counts = br.bodies_ref(now)
    assert (labels == -1).all() and not sizes.any() and counts.tolist() == [0, 0, 0, -1]
    assert [x.tolist() for x in br.never_uploaded(12)] == [labels.tolist(), sizes.tolist(), counts.tolist()]


@pytest.fixture(scope="module")
def expected(sb, oracle):
    """Every stepped case on the oracle, once: {name: (case, {op index: (labels, sizes, counts)}, oracles)}."""
    out = {}
    for case in cs.stepped_cases(sb):
        exp, refs = cs.expected_bodies(oracle, case, before=True)
        out[case["name"]] = (case, exp, refs)
    return out


def test_every_program_runs_on_the_oracle_and_gives_whole_arrays(expected):
    assert len(expected) == 7
    for name, (case, exp, refs) in expected.items():
        n, maxP = len(case["bufs"]), case["cap"][0]
        assert sorted(exp) == [-1] + sorted(case["compare_after"]), name
        for labels, sizes, counts in exp.values():
            assert labels.shape == (n, maxP) and sizes.shape == (n, maxP, 2) and counts.shape == (n, 4), name
            assert labels.dtype == sizes.dtype == counts.dtype == np.int32, name
            for i, b in enumerate(case["bufs"]):
                P = 0 if b is None else b.particle_count
                assert (labels[i] >= 0).sum() == P == sizes[i, :, 0].sum(), (name, i)
                assert counts[i, 0] == (sizes[i, :, 0] > 0).sum() and counts[i, 1] == sizes[i, :, 0].max(), (name, i)
                own = labels[i] == np.arange(maxP)
                assert ((sizes[i, :, 0] > 0) == own).all() and not sizes[i][~own].any(), (name, i)


def test_the_breaking_lattices_come_apart_as_recorded(expected):
    case, exp, refs = expected["yield / break / delete"]
    assert br.brief(exp[-1][2]) == [(1, 144, 0)] * 6
    after_frames, mid_frame = (exp[k][2] for k in case["compare_after"])
    assert after_frames[:, 0].tolist() == [1, 6, 21, 38, 56, 1]
    assert after_frames[:, 1].tolist() == [144, 139, 120, 101, 84, 144]
    assert after_frames[:, 2].tolist() == [0, 5, 18, 33, 53, 0]
    # mid-frame flags are pending, the bodies are those of the last delete pass; the mapping keeps stale entries behind the live slots
    assert any(sr.pending_of(r) > 0 for r in refs) and np.array_equal(mid_frame, after_frames)
    bites = []
    for r, b in zip(refs[1:5], case["bufs"][1:5]):
        now = r.load_buffers(b.copy())
        assert now.beam_count < b.beam_count
        stale = now.copy()
        stale.beam_count = b.beam_count      # the tail behind the live slots read as edges
        bites.append(not np.array_equal(br.bodies_ref(stale)[0], br.bodies_ref(now)[0]))
    assert any(bites), "reading stale mapping entries must give another answer in some scene"


def test_the_default_scene_has_nine_bodies(expected):
    for name in ("default scene, 3 frames", "default scene at 120 / 300"):
        case, exp, refs = expected[name]
        for k in exp:
            assert br.brief(exp[k][2]) == [(9, 40, 2)], (name, k)
    case, exp, refs = expected["default scene, 3 frames"]
    assert case["program"] == [("frame", 3)]


def test_pending_flags_still_connect_and_the_delete_pass_splits(expected):
    case, exp, refs = expected["heterogeneous"]
    a, grabbed, deleted = (exp[k] for k in case["compare_after"])
    whole = [(9, 40, 2), (1, 144, 0), (1, 1024, 0), (1, 2, 0), (0, 0, 0), (0, 0, 0)]
    assert case["program"][-1] == ("delete",) and case["bufs"][5] is None and case["bufs"][4].particle_count == 0
    assert br.brief(exp[-1][2]) == whole and br.brief(a[2]) == whole and br.brief(grabbed[2]) == whole
    assert grabbed[2][:, 3].tolist() == [46, 0, 0, 0, -1, -1]
    assert (grabbed[0][5] == -1).all() and (grabbed[0][4] == -1).all()
    # (the oracle is behind the delete pass here: its mask is clear; the flags were counted by the summary tests, 129 in the lattice)
    assert br.brief(deleted[2])[cs.LATTICE] == (9, 110, 3) and br.brief(deleted[2])[cs.LATTICE] != br.brief(grabbed[2])[cs.LATTICE]
    assert br.brief(deleted[2])[2] == (58, 967, 57)
    assert br.brief(deleted[2])[0] == (9, 40, 2) and br.brief(deleted[2])[3:] == whole[3:]


def test_the_other_cases_bite(expected):
    case, exp, refs = expected["permuted mapping + coincident particles"]
    buf = case["bufs"][0]
    labels = exp[case["compare_after"][0]][0]
    assert buf.mapping[:buf.particle_count].min() >= 50 and (labels[0, :50] == -1).all() and (labels[0, 50:50 + 119] >= 50).all()
    assert not np.array_equal(buf.mapping[:buf.particle_count], np.arange(50, 50 + buf.particle_count))   # data index != slot + 50
    assert br.brief(exp[case["compare_after"][0]][2]) == [(9, 40, 2), (5, 2, 4)]
    case, exp, refs = expected["force saturation"]
    assert case["cap"] == (8, 8) and br.brief(exp[0][2]) == [(1, 2, 0), (3, 2, 0), (1, 2, 0), (3, 2, 0)]
    case, exp, refs = expected["pile"]
    assert case["cap"] == (256, 0) and br.brief(exp[max(exp)][2]) == [(256, 1, 256)]


def test_the_graphs_are_what_they_are_called(sb):
    g = cs.big_graphs(sb)
    for name, (buf, D, counts) in g.items():
        labels, sizes, got = br.bodies_ref(buf)
        assert tuple(got.tolist()) == counts, name
        assert buf.particle_count == 1024 and sorted(buf.mapping[:1024].tolist()) == list(range(1024)), name
        assert not np.array_equal(buf.mapping[:1024], np.arange(1024)), name            # slots != data indices
        assert not np.array_equal(D, np.arange(1024)) and not np.array_equal(buf.mapping[:1024], D), name
    buf, D, _ = g["path"]
    assert buf.beam_count == 1023 and 100 < int(np.argmin(D)) < 924                     # the smallest index inside the path: hooks travel both ways
    a, b = buf.beams["a"], buf.beams["b"]
    live = buf.mapping[1024:1024 + 1023]
    assert not np.array_equal(live, np.sort(live)) and ((a[live] < b[live]).sum() not in (0, 1023))
    buf, D, _ = g["star"]
    assert D[1023] == 1023 and (buf.beams["a"][buf.mapping[1024:1024 + 1023]] == 1023).all()   # the hub at the largest data index
    buf, D, _ = g["pieces"]
    labels, sizes, got = br.bodies_ref(buf)
    assert sorted(sizes[sizes[:, 0] > 0].tolist()) == [[64, 63]] * 16 and got[3] == labels[labels >= 0].min() == 0
    buf, D, _ = g["parallel"]
    labels, sizes, got = br.bodies_ref(buf)
    assert buf.beam_count == 4096 and sorted(sizes[sizes[:, 1] > 0].tolist()) == [[2, 1024], [2, 1024], [3, 2048]]
    for case in cs.graph_cases(sb):
        got = br.bodies_of(case["bufs"], case["cap"][0])[2]
        assert [tuple(r) for r in got.tolist()] == [tuple(c) for c in case["counts"]], case["name"]
        assert len({b.tobytes() for b in got}) > 1, case["name"]                        # a scene of another shape beside the copies
    assert [c["cap"] for c in cs.graph_cases(sb)] == [(1024, 4096), (8, 8), (65, 64)]
