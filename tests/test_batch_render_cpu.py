"""Pictures of a batch (sb_batch_render_device / sb_batch_render_scene) without a GPU: the header declares the two calls, the
library exports them, batch.py binds them with prototypes and a structure of the C struct's size, a NULL handle is refused
before anything touches a device, and the scenes tests/test_gpu_batch_render.py renders give pictures that are not black where
something is expected (so that the GPU comparison cannot pass on black images)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
from render_ref import render_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "softbody.h")
SYMBOLS = ["sb_batch_render_device", "sb_batch_render_scene"]


def nonblack(pic):
    return int((pic != 0).any(axis=-1).sum())


def test_header_declares_and_library_exports_the_render_calls(sb):
    names = sb.engine.declared_symbols()
    L = sb.batch.load_library()
    for s in SYMBOLS:
        assert s in names, s
        assert hasattr(L, s), s
    assert L.sb_abi_version() == 1   # additions only


def test_batch_py_binds_with_prototypes(sb):
    L = sb.batch.load_library()
    vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    po = ctypes.POINTER(sb.batch.SbBatchRenderOptions)
    assert L.sb_batch_render_device.argtypes == [vp, po, vp]
    assert L.sb_batch_render_scene.argtypes == [vp, u32, po, vp, sz]
    for s in SYMBOLS:
        assert getattr(L, s).restype is ctypes.c_int, s
    assert callable(sb.BatchEngine.render) and callable(sb.BatchEngine.render_scene)


def test_max_resolution_is_parsed_from_the_header(sb):
    m = re.search(r"^#define\s+SB_BATCH_RENDER_MAX_RESOLUTION\s+(\d+)\s*$", open(HEADER).read(), re.M)
    assert m and int(m.group(1)) == 1024 == sb.batch.BATCH_RENDER_MAX_RESOLUTION


def test_options_structure_has_the_c_structs_size(sb, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "softbody.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(sb_batch_render_options), '
                   'offsetof(sb_batch_render_options, bounds_size), offsetof(sb_batch_render_options, first), '
                   'offsetof(sb_batch_render_options, reserved)); return 0; }\n')
    exe = str(tmp_path / "size")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    size, o_bounds, o_first, o_reserved = (int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split())
    O = sb.batch.SbBatchRenderOptions
    assert ctypes.sizeof(O) == size == 48
    assert (O.bounds_size.offset, O.first.offset, O.reserved.offset) == (o_bounds, o_first, o_reserved)


def test_null_handle_is_invalid_before_anything_touches_a_device(sb):
    L = sb.batch.load_library()
    o = sb.batch.SbBatchRenderOptions()
    o.struct_size = ctypes.sizeof(o)
    o.resolution = 64
    buf = (ctypes.c_ubyte * (64 * 64 * 3))()
    assert L.sb_batch_render_device(None, None, None) == 1
    assert L.sb_batch_render_device(None, ctypes.byref(o), ctypes.cast(buf, ctypes.c_void_p)) == 1
    assert L.sb_batch_render_scene(None, 0, None, None, 0) == 1
    assert L.sb_batch_render_scene(None, 0, ctypes.byref(o), ctypes.cast(buf, ctypes.c_void_p), len(buf)) == 1


def test_python_checks_resolution_and_range_before_the_library(sb):
    be = sb.BatchEngine.__new__(sb.BatchEngine)
    be._h, be.device, be.n_scenes, be.max_particles, be.max_beams, be._ext_stream = None, 0, 4, 16, 16, None
    import pytest
    for call in (lambda: be.render(1025), lambda: be.render(0), lambda: be.render(64, first=2, count=3),
                 lambda: be.render(64, first=4), lambda: be.render_scene(0, 1025), lambda: be.render(64, out="no")):
        with pytest.raises(ValueError):
            call()


def test_hetero_scenes_give_pictures_that_are_not_black(sb):
    """case_hetero at upload, 64 x 64: the default scene, the 12 x 12 lattice, the 1024-particle lattice, two particles, the empty
    scene (the sixth is never uploaded: black by definition)."""
    bufs = bc.case_hetero(sb)["bufs"]
    assert bufs[5] is None
    assert [nonblack(render_ref(b, 64, 1000.0, 10.0)) for b in bufs[:5]] == [436, 484, 2574, 3, 0]


def test_every_other_rendered_scene_is_not_black_either(sb):
    for case in (bc.case_default(sb, 1), bc.case_default(sb, 2), bc.case_break(sb), bc.case_mapping(sb)):
        for i, b in enumerate(case["bufs"]):
            pic = render_ref(b, 64, 1000.0, 10.0)
            assert nonblack(pic) >= 10, (case["name"], i)
            # (an unstrained beam is white like a disc's ring: at upload a scene may show black and white only)
            assert len(np.unique(pic.reshape(-1, 3), axis=0)) >= 2, (case["name"], i)
    d = bc.case_default(sb, 1)["bufs"][0]
    for S, r in ((400.0, 25.0), (1000.0, 120.0)):   # the wide-primitive settings: discs far over the inline limit
        assert nonblack(render_ref(d, 64, S, r)) > 1000, (S, r)
