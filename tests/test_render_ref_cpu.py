"""tests/render_ref.py (the numpy restatement of host/render.js the GPU picture is checked against) against render.js itself,
byte for byte; and the C declarations of sb_render / sb_render_device / sb_render_options against the ctypes binding."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from render_cases import CASES, custom, shuffled  # noqa: F401  (tests/test_gpu_render.py imports shuffled from here)
from render_ref import ppm, render_ref, v8_hypot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "softbody-webgpu_amd")
DUMP = os.path.join(PKG, "host", "test", "render_dump.js")
HEADER = os.path.join(ROOT, "include", "softbody.h")

needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")


@pytest.fixture(scope="module")
def sbp():
    import __graft_entry__ as ge
    return ge.load_package()


def node_ppm(tmp_path, buf, resolution, bounds_size=None, particle_radius=None):
    d = tmp_path / ("job%d" % len(os.listdir(tmp_path)))
    d.mkdir()
    (d / "mapping.bin").write_bytes(buf.mapping.tobytes())
    (d / "particles.bin").write_bytes(buf.particles.tobytes())
    (d / "beams.bin").write_bytes(buf.beams.tobytes())
    job = {"dir": str(d), "layout": buf.layout, "maxParticles": buf.max_particles, "particleCount": buf.particle_count,
           "beamCount": buf.beam_count, "resolution": resolution, "out": str(d / "out.ppm")}
    if bounds_size is not None:
        job["boundsSize"] = bounds_size
    if particle_radius is not None:
        job["particleRadius"] = particle_radius
    (d / "job.json").write_text(json.dumps(job))
    p = subprocess.run(["node", DUMP, str(d / "job.json")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    return (d / "out.ppm").read_bytes()


def check(tmp_path, buf, resolution=512, bounds_size=None, particle_radius=None):
    want = node_ppm(tmp_path, buf, resolution, bounds_size, particle_radius)
    got = ppm(render_ref(buf, resolution, 1000.0 if bounds_size is None else bounds_size,
                         10.0 if particle_radius is None else particle_radius))
    assert len(got) == len(want)
    if got != want:
        g = np.frombuffer(got, np.uint8)
        w = np.frombuffer(want, np.uint8)
        bad = np.nonzero(g != w)[0]
        raise AssertionError("%d bytes differ from render.js, first at %d: %s vs %s" % (len(bad), bad[0], g[bad[:6]], w[bad[:6]]))
    return np.frombuffer(got, np.uint8)


# ---------------------------------------------------------------- V8's Math.hypot

@needs_node
def test_v8_hypot_restatement(tmp_path):
    rng = np.random.default_rng(5)
    a = rng.normal(0, 1, 200_000) * 10.0 ** rng.integers(-3, 4, 200_000)
    b = rng.normal(0, 1, 200_000) * 10.0 ** rng.integers(-3, 4, 200_000)
    a[:1000] = 0.0
    src = tmp_path / "in.bin"
    np.stack([a, b], 1).astype("<f8").tofile(src)
    js = ("const fs=require('fs');const b=fs.readFileSync(process.argv[1]);const f=new Float64Array(b.buffer,b.byteOffset,b.length/8);"
          "const o=new Float64Array(f.length/2);for(let i=0;i<o.length;i++)o[i]=Math.hypot(f[2*i],f[2*i+1]);"
          "fs.writeFileSync(process.argv[2],Buffer.from(o.buffer));")
    p = subprocess.run(["node", "-e", js, str(src), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    want = np.fromfile(tmp_path / "out.bin", "<f8")
    got = v8_hypot(a, b)
    assert np.array_equal(got.view("u8"), want.view("u8")), "%d of %d differ" % ((got != want).sum(), len(a))
    assert not np.array_equal(np.sqrt(a * a + b * b).view("u8"), want.view("u8")), "the naive form must differ somewhere"


# ---------------------------------------------------------------- scenes against render.js

@needs_node
@pytest.mark.parametrize("layout", [1, 2])
def test_default_scene(sbp, tmp_path, layout):
    buf = sbp.scenes.default_buffers(layout, 256, 512)
    img = check(tmp_path, buf)
    assert (img != 0).sum() > 10000


@needs_node
@pytest.mark.parametrize("res", [1, 7, 500, 513])
def test_resolutions(sbp, tmp_path, res):
    check(tmp_path, sbp.scenes.default_buffers(1, 256, 512), res)


@needs_node
def test_bounds_and_radius(sbp, tmp_path):
    buf = sbp.scenes.default_buffers(2, 256, 512)
    check(tmp_path, buf, 300, bounds_size=1234.5, particle_radius=17.3)
    check(tmp_path, buf, 257, bounds_size=700.0, particle_radius=3.0)


def check_case(sbp, tmp_path, name, layout=None):
    """Every picture the case names, against render.js."""
    case = CASES[name]
    buf = case.buffers(sbp, layout)
    return [check(tmp_path, buf, res, bounds_size=S, particle_radius=r) for res, S, r in case.renders]


@needs_node
@pytest.mark.parametrize("layout", [1, 2])
def test_edges(sbp, tmp_path, layout):
    """Discs cut by every edge and corner, beams that enter, leave and cross the image on every side."""
    check_case(sbp, tmp_path, "edges", layout)


@needs_node
def test_slot_order_decides(sbp, tmp_path):
    """Crossing beams of different stress and overlapping discs: the later slot is on top, inner versus ring included."""
    a, = check_case(sbp, tmp_path, "slot_order", 1)
    # the same with the slots reversed gives another picture
    b, = check_case(sbp, tmp_path, "slot_order_reversed", 1)
    assert not np.array_equal(a, b)


@needs_node
def test_nonfinite_strain_stress(sbp, tmp_path):
    check_case(sbp, tmp_path, "nonfinite_colours", 2)


@needs_node
@pytest.mark.parametrize("layout", [1, 2])
def test_shuffled_mapping(sbp, tmp_path, layout):
    check_case(sbp, tmp_path, "shuffled_mapping", layout)


@needs_node
def test_lattice_small_pixels(sbp, tmp_path):
    """Config 2's regime: discs and beams of about a pixel (a jittered lattice at large bounds)."""
    buf = sbp.scenes.lattice_buffers(60, 40, d=30.0, origin=(40.0, 40.0), layout=2, jitter=3.0)
    buf.beams["stress"][:buf.beam_count] = np.linspace(-1.0, 1.0, buf.beam_count, dtype="f4")
    check(tmp_path, buf, 256, bounds_size=2000.0)


# ---------------------------------------------------------------- the C ABI

def test_header_declares_render():
    import re
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"sb_status\s+sb_render\s*\(\s*sb_engine\s*\*\s*e\s*,\s*const\s+sb_render_options\s*\*", src)
    assert re.search(r"sb_status\s+sb_render_device\s*\(\s*sb_engine\s*\*\s*e\s*,\s*const\s+sb_render_options\s*\*", src)
    assert "typedef struct sb_render_options" in src
    assert "SB_ABI_VERSION 1" in src


def test_render_options_layout_matches_c(sbp, tmp_path):
    import ctypes
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "softbody.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
                     " sizeof(sb_render_options), offsetof(sb_render_options, struct_size), offsetof(sb_render_options, resolution),"
                     " offsetof(sb_render_options, bounds_size), offsetof(sb_render_options, particle_radius),"
                     " offsetof(sb_render_options, reserved)); return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R = sbp.engine.SbRenderOptions
    want = [ctypes.sizeof(R), R.struct_size.offset, R.resolution.offset, R.bounds_size.offset, R.particle_radius.offset,
            R.reserved.offset]
    assert got == want
