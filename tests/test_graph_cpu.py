"""tests/graph_ref.py, the numpy restatement of sb_batch_graph_device, on hand-built graphs whose five arrays are
written out by hand; csrc/sb_graph_math.h on the host (tests/graph_check.cpp, `make hostcheck`); the binding's field names."""
import os
import subprocess

import numpy as np
import pytest

import graph_ref as ref
from graph_cases import corner_scenes, scene
from test_hostcheck_cpu import CSRC, ENV


def test_chain(sb):
    g = ref.graph_ref(scene(sb, (6, 5), 4, [(0, 1), (1, 2), (2, 3)]))
    assert g.ends.tolist() == [[0, 1], [1, 2], [2, 3], [-1, -1], [-1, -1]]
    assert g.row_ptr.tolist() == [0, 1, 3, 5, 6, 6, 6]
    assert g.nbr.tolist() == [[1, 0], [0, 0], [2, 1], [1, 1], [3, 2], [2, 2]] + [[-1, -1]] * 4
    assert g.counts.tolist() == [3, 4, 2, 1]
    assert g.material[:3].tolist() == [[10.0, 50.0, 700.0, np.float32(0.2), 1.0e9]] * 3 and not g.material[3:].any()
    assert [a.dtype for a in g] == [np.int32, np.float32, np.int32, np.int32, np.int32]


def test_star_with_the_hub_as_high_endpoint(sb):
    """the hub is the record's b in two of its three beams: the neighbour is the OTHER endpoint whichever half holds the hub"""
    g = ref.graph_ref(scene(sb, (4, 4), 4, [(1, 0), (0, 2), (3, 0)]))
    assert g.ends.tolist() == [[1, 0], [0, 2], [3, 0], [-1, -1]]
    assert g.row_ptr.tolist() == [0, 3, 4, 5, 6]
    assert g.nbr.tolist() == [[1, 0], [2, 1], [3, 2], [0, 0], [0, 1], [0, 2], [-1, -1], [-1, -1]]
    assert g.counts.tolist() == [3, 4, 3, 0]


def test_parallel_beams_and_a_tie_of_degrees(sb):
    """two beams on one pair are two edges; both ends have degree 2: the smaller data index is named"""
    g = ref.graph_ref(scene(sb, (4, 3), 3, [(2, 1), (1, 2)], lengths=[10.0, 12.0]))
    assert g.ends.tolist() == [[2, 1], [1, 2], [-1, -1]]
    assert g.row_ptr.tolist() == [0, 0, 2, 4, 4]
    assert g.nbr.tolist() == [[2, 0], [2, 1], [1, 0], [1, 1], [-1, -1], [-1, -1]]
    assert g.counts.tolist() == [2, 2, 2, 1]
    assert g.material[:, 0].tolist() == [10.0, 12.0, 0.0]


def test_sparse_out_of_order_mapping(sb):
    """particle slots 0, 1, 2 at data indices 5, 0, 3; beam slots 0, 1 at data indices 6, 2: everything is named by DATA index, the
    rows of nbr by ascending beam data index -- slot 1's beam first"""
    buf = scene(sb, (8, 8), 3, [(0, 1), (0, 2)], layout=2, pmap=[5, 0, 3], bmap=[6, 2])
    g = ref.graph_ref(buf)
    ends = np.full((8, 2), -1)
    ends[6], ends[2] = (5, 0), (5, 3)
    assert g.ends.tolist() == ends.tolist()
    assert g.row_ptr.tolist() == [0, 1, 1, 1, 2, 2, 4, 4, 4]
    assert g.nbr.tolist() == [[5, 6], [5, 2], [3, 2], [0, 6]] + [[-1, -1]] * 12
    assert g.counts.tolist() == [2, 3, 2, 5]
    # a stale mapping entry behind beam_count is no edge; a dropped data index (SKIP_PENDING) is not listed
    buf.mapping[8 + 2] = 7
    assert not ref.same(ref.graph_ref(buf), g)
    h = ref.graph_ref(buf, drop=[6])
    assert h.ends[6].tolist() == [-1, -1] and h.nbr[:3].tolist() == [[5, 2], [3, 2], [-1, -1]] and h.counts.tolist() == [1, 2, 1, 3]


def test_self_loop(sb):
    """a beam from a particle to itself is two half-edges at it: side 0, then side 1"""
    g = ref.graph_ref(scene(sb, (2, 2), 2, [(1, 1)]))
    assert g.row_ptr.tolist() == [0, 0, 2] and g.nbr.tolist() == [[1, 0], [1, 0], [-1, -1], [-1, -1]] and g.counts.tolist() == [1, 1, 2, 1]


def test_empty_scene_and_stacking(sb):
    empty = ref.graph_ref(scene(sb, (4, 4), 3, []))
    assert not ref.same(empty, ref.never_uploaded(4, 4))
    assert empty.counts.tolist() == [0, 0, 0, -1] and (empty.ends == -1).all() and (empty.nbr == -1).all() and not empty.row_ptr.any()
    g = ref.graph_of([scene(sb, (4, 4), 4, [(0, 1)]), None], 4, 4)
    assert [a.shape for a in g] == [(2, 4, 2), (2, 4, 5), (2, 5), (2, 8, 2), (2, 4)]
    assert g.counts.tolist() == [[1, 2, 1, 0], [0, 0, 0, -1]]
    assert ref.same(g, ref.graph_of([None, None], 4, 4)) == ["ends", "material", "row_ptr", "nbr", "counts"]


def test_corner_scenes(sb):
    """the scenes of the GPU test's capacity corners: the star's hub has degree 4096, in ascending order of beam data index"""
    bufs = corner_scenes(sb)
    g = ref.graph_of(bufs, 1024, 4096)
    assert g.counts.tolist() == [[4096, 1024, 4096, 0], [1, 2, 1, 0], [0, 0, 0, -1], [0, 0, 0, -1], [64, 65, 2, 1]]
    assert g.row_ptr[0, :3].tolist() == [0, 4096, 4101] and g.nbr[0, :4096, 1].tolist() == list(range(4096))
    assert g.nbr[0, :4, 0].tolist() == [1, 2, 3, 4] and g.nbr[0, 4096:4101].tolist() == [[0, 0], [0, 1023], [0, 2046], [0, 3069], [0, 4092]]
    assert g.ends[0, :4].tolist() == [[1, 0], [0, 2], [0, 3], [4, 0]] and g.material[0, 100, 0] == 13.0
    assert g.nbr[4, 62:66].tolist() == [[32, 31], [31, 31], [33, 32], [32, 32]] and g.ends[1, 0].tolist() == [1, 0]


def test_binding_names(sb):
    assert sb.batch.GRAPH_COUNT_FIELDS == sb.GRAPH_COUNT_FIELDS and len(sb.GRAPH_COUNT_FIELDS) == ref.COUNT_WORDS == sb.batch.GRAPH_COUNT_WORDS
    assert sb.GRAPH_MATERIAL_FIELDS == ref.MATERIAL_FIELDS and len(ref.MATERIAL_FIELDS) == sb.batch.GRAPH_MATERIAL_WORDS
    assert sb.batch.Graph._fields == ref.Graph._fields
    assert "sb_batch_graph_device" in sb.engine.declared_symbols()


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_key_codec_under_sanitizers(san):
    """csrc/sb_graph_math.h (tests/graph_check.cpp): the key round-trips over the corner values, key order is (particle, beam, side)
    order, the bitonic network sorts a star, self-loops, a chain and random scenes as std::sort does, lower_bound is the prefix sum"""
    target = os.path.join("hostcheck_build", "graph_check_" + san)
    p = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([os.path.join(CSRC, target)], capture_output=True, text=True, timeout=300, env=ENV)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and p.stdout.startswith("GRAPH_CHECK_OK 26244 10"), (p.stdout, p.stderr[-3000:])
