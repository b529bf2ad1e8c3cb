"""Engine.bodies() (sb_bodies / sb_bodies_device) without a GPU: the header declares the calls, the library exports
them, engine.py binds them with a structure of the C struct's size, a NULL handle is refused before anything touches a device,
every case of tests/test_gpu_bodies.py BITES on the oracle alone, and no kernel of the call spills or uses scratch."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_bodies_ref as br  # noqa: E402
import bodies_cases as bc  # noqa: E402
import summary_cases as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sb_bodies", "sb_bodies_device"]


def test_header_declares_and_library_exports_the_calls(sb):
    names = sb.engine.declared_symbols()
    L = sb.engine.load_library()
    for s in SYMBOLS:
        assert s in names, s
        assert hasattr(L, s), s
    assert L.sb_abi_version() == 1   # additions only
    vp, po = ctypes.c_void_p, ctypes.POINTER(sb.engine.SbBodiesOptions)
    assert L.sb_bodies_device.argtypes == [vp, po, vp, vp, vp] and L.sb_bodies.argtypes == [vp, po, vp, vp, vp]
    assert callable(sb.Engine.bodies) and callable(sb.Engine.bodies_host)


def test_options_structure_and_words_are_the_c_headers(sb, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "softbody.h"\n'
                   'int main(void) { printf("%zu %zu %u %u\\n", sizeof(sb_bodies_options), offsetof(sb_bodies_options, reserved), '
                   'SB_BODY_WORDS, SB_BATCH_BODY_WORDS); return 0; }\n')
    exe = str(tmp_path / "size")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    size, o_reserved, words, batch_words = (int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split())
    O = sb.engine.SbBodiesOptions
    assert ctypes.sizeof(O) == size == 32 and O.reserved.offset == o_reserved == 4
    assert words == batch_words == sb.engine.BODY_WORDS == len(sb.engine.BODY_FIELDS) == br.WORDS


def test_field_names_are_the_batchs_not_a_copy(sb):
    assert sb.engine.BODY_FIELDS is sb.batch.BODY_FIELDS


def test_null_handle_is_invalid_before_anything_touches_a_device(sb):
    L = sb.engine.load_library()
    labels, counts = (ctypes.c_int32 * 8)(), (ctypes.c_int64 * 4)()
    o = sb.engine.SbBodiesOptions()
    o.struct_size = ctypes.sizeof(o)
    vp = ctypes.c_void_p
    assert L.sb_bodies(None, None, None, None, None) == 1
    assert L.sb_bodies(None, ctypes.byref(o), ctypes.cast(labels, vp), None, ctypes.cast(counts, vp)) == 1
    assert L.sb_bodies_device(None, None, None, None, None) == 1
    assert L.sb_bodies_device(None, ctypes.byref(o), ctypes.cast(labels, vp), None, None) == 1


def brief(counts):
    return tuple(int(x) for x in counts)


def check_shape(case, exp):
    """what the definition says of ANY answer: labels -1 exactly where no particle lives, a label is a root, sizes add up"""
    buf = case["buf"]
    lives = np.zeros(buf.max_particles, bool)
    lives[buf.mapping[:buf.particle_count].astype(np.int64)] = True
    for k, (labels, sizes, counts) in exp.items():
        assert np.array_equal(labels >= 0, lives), (case["name"], k)
        roots = np.flatnonzero(labels == np.arange(buf.max_particles))
        assert np.array_equal(np.unique(labels[lives]), roots) and len(roots) == counts[0], (case["name"], k)
        assert sizes[:, 0].sum() == buf.particle_count and not sizes[np.setdiff1d(np.arange(buf.max_particles), roots)].any()
        assert counts.dtype == np.int64


def test_default_scene_is_nine_bodies(sb, oracle):
    for mode in (sc.ALLPAIRS, sc.OFF):
        case = bc.case_default(sb, mode)
        exp = bc.expected_cached(oracle, case)
        assert sorted(exp) == [-1, 0, 1]
        check_shape(case, exp)
        assert exp[-1][2][0] == 9 and 1 < exp[-1][2][1] < case["buf"].particle_count   # neither one body nor all single
        assert not np.array_equal(exp[-1][0][:119], np.arange(119))


def pending_after_first_op(oracle, case):
    ref = sc.make_oracle(oracle, case)
    sc.apply_to_oracle(ref, case["program"][0])
    return sc.sr.pending_of(ref)


def test_breaking_case_is_one_body_with_flags_pending_and_loses_beams_to_the_pass(sb, oracle):
    """summary_cases.case_break: the 12 beams flagged at substep 40 still connect; the delete pass removes them, which the sizes
    show while the lattice is still one body; the frame after leaves it in pieces"""
    case = bc.case_break(sb)
    exp = bc.expected_cached(oracle, case)
    check_shape(case, exp)
    assert pending_after_first_op(oracle, case) == 12
    assert brief(exp[0][2]) == (1, 144, 0, 0) and exp[0][1][0].tolist() == [144, 385]
    assert brief(exp[1][2]) == (1, 144, 0, 0) and exp[1][1][0].tolist() == [144, 373]
    assert brief(exp[2][2]) == (3, 142, 2, 1)


def test_break_apart_case_is_in_pieces_by_the_delete_pass_alone(sb, oracle):
    case = bc.case_break_apart(sb)
    exp = bc.expected_cached(oracle, case)
    check_shape(case, exp)
    assert pending_after_first_op(oracle, case) == 34
    assert brief(exp[0][2]) == (1, 144, 0, 0)
    assert brief(exp[1][2]) == (4, 141, 3, 1) and exp[1][1][:, 1].sum() == 385 - 34


def test_capacity_case_leaves_most_rows_empty(sb, oracle):
    case = bc.case_capacity(sb)
    exp = bc.expected_cached(oracle, case)
    check_shape(case, exp)
    labels, sizes, counts = exp[-1]
    assert brief(counts) == (1, 48, 0, 50) and (labels == -1).sum() == 5000 - 48
    assert labels.max() < 200 and np.flatnonzero(sizes.any(axis=1)).tolist() == [50]


def test_cut_lattice_falls_in_two(sb):
    whole, cut = bc.cut_lattice(sb)
    assert brief(br.bodies_ref(whole)[2]) == (1, 288, 0, 0)
    labels, sizes, counts = br.bodies_ref(cut)
    assert brief(counts) == (2, 144, 0, 0) and len(np.unique(labels)) == 2     # equal sizes: the smaller label, 0, wins
    assert sizes[:, 1].sum() == cut.beam_count < whole.beam_count


@pytest.mark.parametrize("name", list(bc.GRAPHS))
def test_graph_is_what_its_construction_says_and_shuffled(sb, oracle, name):
    case = bc.graph_case(sb, name)
    buf, D = case["buf"], case["D"]
    exp = bc.expected_cached(oracle, case)
    check_shape(case, exp)
    labels, sizes, counts = exp[-1]
    assert brief(counts) == case["counts"], (name, brief(counts))
    P, B, maxP = buf.particle_count, buf.beam_count, buf.max_particles
    assert P > 1024 and sizes[:, 1].sum() == B                       # beyond one workgroup of the batch's kernel
    for m, n in ((buf.mapping[:P], P), (buf.mapping[maxP:maxP + B], B)):
        assert not np.array_equal(m, np.arange(n)) and not np.array_equal(np.sort(m), m)
    assert not np.array_equal(D, np.arange(P))
    a, b = buf.beams["a"][buf.mapping[maxP:maxP + B].astype(np.int64)].astype(np.int64), buf.beams["b"][buf.mapping[maxP:maxP + B].astype(np.int64)].astype(np.int64)
    if name.startswith("path") or name.startswith("16 pieces"):      # the beams of a path really are 30 long
        d = buf.particles[a, :2] - buf.particles[b, :2]
        assert np.array_equal(np.abs(d).sum(axis=1), np.full(B, 30.0, "f4"))
    if name.startswith("star"):
        hub = int(D.max())
        assert np.all((a == hub) | (b == hub)) and labels[hub] == D.min() != hub


def test_no_kernel_of_the_bodies_spills_or_uses_scratch():
    """the compiler's own report (tools/kernel_resources.py) for every kernel of sb_bodies.hip, and the committed table is that report"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                        os.path.join(ROOT, "softbody-webgpu_amd", "csrc", "sb_bodies.hip"), "k_bodies"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    rows = [ln.split() for ln in p.stdout.splitlines() if "k_bodies" in ln]
    names = " ".join(" ".join(r) for r in rows)
    for k in ("k_bodies_init", "k_bodies_union", "k_bodies_flatten<true>", "k_bodies_flatten<false>", "k_bodies_beams", "k_bodies_roots",
              "k_bodies_counts"):
        assert k in names, k
    assert len(rows) == 7
    for r in rows:
        assert r[r.index("spill") + 1] == "0" and r[r.index("scratch") + 1] == "0", r
    assert p.stdout == open(os.path.join(ROOT, "profiles", "bodies_kernel_resources.txt")).read()
