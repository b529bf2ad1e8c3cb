"""Scenes of the tests of Engine.contacts() (sb_contacts_device), shared by tests/test_contacts_cpu.py (the
reference alone: what every scene must show) and tests/test_gpu_contacts.py.  A scene is a dict: name, buf, bounds, radius.  The
scenes built here are uploaded and not stepped; every mapping is shuffled as in bodies_cases.graph_scene: particle NUMBER k lives
at data index D[k] in slot S[k], two independent random draws."""
import numpy as np

import batch_contacts_cases as bcc
import contacts_ref as cref

SCAN_BLOCK = 1024       # SBC_SCAN of sb_contacts.hip: the words a workgroup of the cell scan owns


def cells_per_side(bounds, radius, particles):
    """contacts_cells_per_side as sb_contacts.hip's rule gives it: floor(bounds / (2r (1 + 1/64))), at least 1, at most the
    largest G with G^2 <= 8 particles"""
    f = np.float32
    cell_min = f(radius) * f(2.0) * (f(1.0) + f(1.0) / f(64.0))
    cap = 1
    while (cap + 1) ** 2 <= 8 * max(particles, 1) and cap < 8192:
        cap += 1
    per_side = f(bounds) / cell_min
    return int(min(cap, max(1, int(per_side))))


def free_scene(sb, cap, pts, seed, max_beams=4):
    """len(pts) free particles: number k at data index D[k] in slot S[k].  Returns (Buffers, D)."""
    pts = np.asarray(pts, "f4")
    n = len(pts)
    rng = np.random.default_rng(seed)
    D, S = rng.permutation(cap)[:n], rng.permutation(n)
    buf = sb.Buffers(2, cap, max_beams)
    buf.particles[D, :2] = pts[:, :2]
    buf.mapping[S] = D
    buf.particle_count, buf.beam_count = n, 0
    return buf, D


def jittered_grid(n, per_row, origin, seed, spacing=20.0, jitter=0.5):
    """n points on rows of per_row, `spacing` apart, each moved by up to `jitter` in x and y: neighbours 19 - 21 apart at the
    defaults, so about half of the neighbouring pairs touch (2r = 20)"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    pts = np.zeros((n, 2), "f4")
    pts[:, 0] = origin[0] + spacing * (k % per_row)
    pts[:, 1] = origin[1] + spacing * (k // per_row)
    return (pts + rng.uniform(-jitter, jitter, (n, 2))).astype("f4")


def _scene(name, buf, bounds, radius=10.0, **kw):
    return dict(name=name, buf=buf, bounds=float(bounds), radius=float(radius), **kw)


def pile_4097(sb):
    """4097 particles at capacity 5000: more than one workgroup, more than one block of the 64-bit scan over the data indices
    (4096 + 1), pairs on both sides of the 256- and the 4096-index boundaries"""
    buf, D = free_scene(sb, 5000, jittered_grid(4097, 65, (40.0, 40.0), seed=21), seed=22)
    return _scene("pile 4097 in 5000", buf, 2000.0, D=D)


def box_16384(sb):
    """16 384 particles over a box of 6000: 295 cells per side, 87 026 count words = 85 blocks of the cell scan"""
    buf, D = free_scene(sb, 16384, jittered_grid(16384, 128, (1500.0, 1500.0), seed=23), seed=24)
    return _scene("box 16384", buf, 6000.0, D=D)


def scan_edge(sb, g):
    """A scene of g cells per side, g^2 a multiple of the scan block: the count words are g^2 + 1, ONE more than whole blocks (the
    last word alone in its block).  g^2 + 1 itself is never a multiple of a block of 1024: a square is 0 or 1 modulo 4."""
    n = {32: 200, 64: 600}[g]
    bounds = {32: 655.0, 64: 1310.0}[g]
    rng = np.random.default_rng(30 + g)
    pts = np.zeros((n, 2), "f4")
    pts[:n // 2] = jittered_grid(n // 2, 10, (bounds - 215.0, bounds - 20.0 * (n // 20) - 15.0), seed=g)   # into the last cells
    pts[n // 2:] = rng.uniform(5.0, bounds - 5.0, (n - n // 2, 2))
    buf, D = free_scene(sb, n + 24, pts, seed=31 + g)
    return _scene("%d cells per side" % g, buf, bounds, D=D, cells=g)


def crowd_600(sb):
    """600 particles inside ONE cell (an 18 x 18 patch inside the cell 24, 24 of 49): every particle has hundreds of partners, the
    list sweeps run far more than four partners above"""
    rng = np.random.default_rng(41)
    pts = (491.0 + 18.0 * rng.random((600, 2))).astype("f4")
    buf, D = free_scene(sb, 700, pts, seed=42)
    return _scene("crowd 600", buf, 1000.0, D=D)


BIG = {"pile 4097 in 5000": pile_4097, "box 16384": box_16384, "32 cells per side": lambda sb: scan_edge(sb, 32),
       "64 cells per side": lambda sb: scan_edge(sb, 64), "crowd 600": crowd_600}
_cache = {}


def big_scene(sb, name):
    if name not in _cache:
        _cache[name] = BIG[name](sb)
    return _cache[name]


def batch_scenes(sb):
    """Every uploaded scene of batch_contacts_cases.all_cases as a scene of its own: (case name / scene number, buf, bounds, radius,
    finite); scenes that occur in several cases once."""
    out, seen = [], set()
    for case in bcc.all_cases(sb):
        radius, bounds = bcc.geometry(case)
        for i, buf in enumerate(case["bufs"]):
            if buf is None:
                continue
            key = (buf.particles.tobytes(), buf.mapping.tobytes(), buf.particle_count, radius, bounds)
            if key in seen:
                continue
            seen.add(key)
            P = buf.particle_count
            finite = bool(np.isfinite(buf.particles[buf.mapping[:P].astype(np.int64), :2]).all())
            out.append(_scene("%s / %d" % (case["name"], i), buf, bounds, radius, finite=finite, fits_batch=buf.max_particles <= 1024))
    return out


def for_engine(sb, buf):
    """`buf` as an Engine takes it: a beam capacity of at least one"""
    if buf.max_beams > 0:
        return buf
    out = sb.Buffers(buf.layout, buf.max_particles, 4)
    out.particles[:] = buf.particles
    out.mapping[:buf.max_particles] = buf.mapping[:buf.max_particles]
    out.metadata[12:28] = buf.metadata[12:28]
    out.particle_count, out.beam_count = buf.particle_count, 0
    return out


def striped_labels(max_particles, width=3):
    """a partition of the caller's own: data indices in stripes of `width`"""
    return (np.arange(max_particles) // width % 5 - 2).astype(np.int32)     # (negative labels too: only ever compared)


_ref_cache = {}


def expected(scene, labels=None, max_pairs=0, other_body=False, key=None):
    """contacts_ref of the scene as uploaded, computed once per (scene, key) and shared; the arrays are not to be written to"""
    k = (scene["name"], key, max_pairs, other_body)
    if key is None or k not in _ref_cache:
        out = cref.contacts_ref(scene["buf"], scene["radius"], scene["bounds"], labels, max_pairs, other_body)
        for a in out:
            a.setflags(write=False)
        if key is None:
            return out
        _ref_cache[k] = out
    return _ref_cache[k]
