"""tests/render_ref.py (the numpy restatement of host/render.js the GPU picture is checked against) against render.js itself,
byte for byte; and the C declarations of sb_render / sb_render_device / sb_render_options against the ctypes binding."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

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


def custom(sbp, layout, points, beams):
    """points: [(x, y)]; beams: [(a, b, strain, stress)] (data indices = slots)."""
    from softbody_webgpu_amd.layout import BEAM_DTYPE, Buffers
    buf = Buffers(layout, max(len(points), 1) + 3, max(len(beams), 1) + 3)
    b = np.zeros(len(beams), dtype=BEAM_DTYPE[layout])
    for i, (a, c, sn, ss) in enumerate(beams):
        b[i]["a"], b[i]["b"], b[i]["strain"], b[i]["stress"] = a, c, sn, ss
        b[i]["length"] = b[i]["target_length"] = 1.0
    buf.set_scene(np.asarray(points, dtype="<f4"), b)
    return buf


def shuffled(buf, seed):
    """Slots != data indices: particles and beams moved to permuted data indices, both mappings permuted."""
    out = buf.copy()
    rng = np.random.default_rng(seed)
    P, B, maxP = buf.particle_count, buf.beam_count, buf.max_particles
    pp = rng.permutation(buf.max_particles)[:P]
    bp = rng.permutation(buf.max_beams)[:B]
    out.particles[:] = 0
    out.particles[pp] = buf.particles[:P]
    bb = buf.beams[:B].copy()
    bb["a"] = pp[bb["a"]]
    bb["b"] = pp[bb["b"]]
    out.beams[:] = 0
    out.beams[bp] = bb
    sp, sbm = rng.permutation(P), rng.permutation(B)
    out.mapping[:P] = pp[sp]
    out.mapping[maxP:maxP + B] = bp[sbm]
    return out


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


@needs_node
@pytest.mark.parametrize("layout", [1, 2])
def test_edges(sbp, tmp_path, layout):
    """Discs cut by every edge and corner, beams that enter, leave and cross the image on every side."""
    pts = [(-5.0, 500.0), (1005.0, 500.0), (500.0, -4.0), (500.0, 1006.0), (2.0, 3.0), (998.0, 997.0), (-8.0, 1007.0), (1009.0, -9.0),
           (-300.0, 200.0), (1300.0, 800.0), (200.0, -400.0), (800.0, 1500.0), (-50.0, -70.0), (1100.0, 1200.0), (400.0, 400.0),
           (-2000.0, 500.5), (3000.0, 499.5)]
    bms = [(8, 9, 0.1, 0.3), (10, 11, -0.2, -0.4), (12, 13, 0.5, 0.9), (14, 8, 0.0, 0.0), (14, 11, 1.5, -1.5), (15, 16, 0.25, 0.25),
           (0, 1, 0.3, 0.6), (2, 3, 0.7, -0.7), (6, 7, 0.05, 0.1), (9, 8, 0.2, 0.2)]
    buf = custom(sbp, layout, pts, bms)
    check(tmp_path, buf, 128)
    check(tmp_path, buf, 97, particle_radius=33.0)


@needs_node
def test_slot_order_decides(sbp, tmp_path):
    """Crossing beams of different stress and overlapping discs: the later slot is on top, inner versus ring included."""
    pts = [(500.0, 500.0), (507.0, 503.0), (512.0, 498.0), (100.0, 100.0), (900.0, 900.0), (100.0, 900.0), (900.0, 100.0),
           (300.0, 300.0), (300.0, 700.0)]
    bms = [(3, 4, 0.1, -0.9), (5, 6, 0.6, 0.9), (7, 8, 0.0, 0.3), (8, 7, 0.9, -0.3)]
    buf = custom(sbp, 1, pts, bms)
    a = check(tmp_path, buf, 200)
    # the same with the slots reversed gives another picture
    rev = buf.copy()
    P, B, maxP = buf.particle_count, buf.beam_count, buf.max_particles
    rev.mapping[:P] = buf.mapping[:P][::-1]
    rev.mapping[maxP:maxP + B] = buf.mapping[maxP:maxP + B][::-1]
    b = check(tmp_path, rev, 200)
    assert not np.array_equal(a, b)


@needs_node
def test_nonfinite_strain_stress(sbp, tmp_path):
    nan, inf = float("nan"), float("inf")
    pts = [(100.0 + 80.0 * i, 100.0 + 60.0 * (i % 3)) for i in range(12)] + [(100.0 + 80.0 * i, 800.0) for i in range(12)]
    vals = [(nan, 0.0), (0.0, nan), (inf, 0.0), (-inf, 0.0), (0.0, inf), (0.0, -inf), (nan, nan), (inf, -inf), (1e30, -1e30),
            (-0.0, -0.0), (0.5, 1e-8), (-3.0, -2.0)]
    bms = [(i, 12 + i, sn, ss) for i, (sn, ss) in enumerate(vals)]
    check(tmp_path, custom(sbp, 2, pts, bms), 160)


@needs_node
@pytest.mark.parametrize("layout", [1, 2])
def test_shuffled_mapping(sbp, tmp_path, layout):
    buf = sbp.scenes.default_buffers(layout, 256, 512)
    buf.beams["strain"][:buf.beam_count] = np.linspace(-1.5, 1.5, buf.beam_count, dtype="f4")
    buf.beams["stress"][:buf.beam_count] = np.linspace(1.2, -1.2, buf.beam_count, dtype="f4")
    check(tmp_path, shuffled(buf, 9), 400)


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
