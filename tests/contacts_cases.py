"""Scenes of the tests of Engine.contacts() (sb_contacts_device), shared by tests/test_contacts_cpu.py (the
reference alone: what every scene must show) and tests/test_gpu_contacts.py.  A scene is a dict: name, buf, bounds, radius.  The
scenes built here are uploaded and not stepped; every mapping is shuffled as in bodies_cases.graph_scene: particle NUMBER k lives
at data index D[k] in slot S[k], two independent random draws."""
import numpy as np

import batch_contacts_cases as bcc
import contacts_ref as cref

SCAN_BLOCK = 1024       # SBQ_SCAN of sb_report.h: the words a workgroup of the scan owns
SCAN_SUMS = 256         # SBQ_BLOCK: the block sums one trip of k_report_scan_sums' loop takes
SECOND_TRIP = SCAN_BLOCK * SCAN_SUMS     # the first word whose block sum the SECOND trip of that loop owns: 2^18


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


def cell_words(scene):
    """(G, cell [P]): the cells per side and the count word y * G + x of every particle NUMBER, by sb_contacts.hip's rule in
    float32 (sb_batch_cell_geometry's side, sb_grid_coord's division and clamp); finite positions"""
    f = np.float32
    buf, D = scene["buf"], scene["D"]
    G = cells_per_side(scene["bounds"], scene["radius"], buf.particle_count)
    side = max(f(scene["radius"]) * f(2.0) * (f(1.0) + f(1.0) / f(64.0)), f(scene["bounds"]) / f(G))
    q = (buf.particles[D, :2].astype(f) / f(side)).astype(f)
    c = np.where(q > 0, np.minimum(q, f(G - 1)), f(0)).astype(np.int64)       # (truncation; q >= G clamps to G - 1)
    return G, c[:, 1] * G + c[:, 0]


def scan_model(words, carry=True):
    """The exclusive scan of `words` the way the three launches of sbc_scan / sby_scan take it, in integers: a sum per block of
    SCAN_BLOCK words; the block sums scanned SCAN_SUMS at a time with a running carry between the trips; added back inside every
    block.  carry=False is the loop with its carry LEFT OUT: what a test scene must tell from the right answer.  (out, total)"""
    w = np.asarray(words, dtype=np.int64)
    nb = (len(w) + SCAN_BLOCK - 1) // SCAN_BLOCK
    blocks = np.zeros(nb * SCAN_BLOCK, np.int64)
    blocks[:len(w)] = w
    blocks = blocks.reshape(nb, SCAN_BLOCK)
    bsum = blocks.sum(axis=1)
    base, run = np.zeros(nb, np.int64), 0
    for at in range(0, nb, SCAN_SUMS):
        part = bsum[at:at + SCAN_SUMS]
        base[at:at + SCAN_SUMS] = (run if carry else 0) + np.cumsum(part) - part
        run += int(part.sum())
    out = base[:, None] + np.cumsum(blocks, axis=1) - blocks
    return out.reshape(-1)[:len(w)], run


def free_scene(sb, cap, pts, seed, max_beams=4, among=None):
    """len(pts) free particles: number k at data index D[k] in slot S[k].  among: the data indices to draw from (all of the
    capacity's where None).  Returns (Buffers, D)."""
    pts = np.asarray(pts, "f4")
    n = len(pts)
    rng = np.random.default_rng(seed)
    D = rng.permutation(cap)[:n] if among is None else np.asarray(among, np.int64)[rng.permutation(len(among))[:n]]
    S = rng.permutation(n)
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


def cells_544(sb):
    """40 000 particles over a box of 11 060: 544 cells per side, 295 937 count words = 290 blocks of the cell scan, so the SECOND
    trip of the loop over the block sums owns the cells from word 2^18 = row 481, column 480 on.  Three jittered patches -- the
    low rows, twenty rows across that word (whose own row the patch spans from x = 500 to 10 500), the last rows up to the last
    cell -- and 15 000 particles scattered over the whole box"""
    bounds = 11060.0
    rng = np.random.default_rng(61)
    pts = np.concatenate([jittered_grid(10000, 200, (100.0, 100.0), seed=62),
                          jittered_grid(10000, 500, (500.0, 9600.0), seed=63),
                          jittered_grid(5000, 100, (bounds - 1990.0, bounds - 990.0), seed=64),
                          rng.uniform(5.0, bounds - 5.0, (15000, 2)).astype("f4")])
    buf, D = free_scene(sb, 40100, pts, seed=65)
    return _scene("544 cells per side", buf, bounds, D=D, cells=544, prune=True)


def indices_past_2_18(sb):
    """6000 particles on a jittered grid at capacity 2^18 + 4096: 260 blocks of the 64-bit scan over the data indices.  The data
    indices are drawn from every 64th index below 2^18 and every index from 2^18 on, so about half of the particles -- and of the
    pairs, which are listed under their smaller index -- lie in the second trip's four blocks"""
    cap = SECOND_TRIP + 4096
    among = np.concatenate([np.arange(0, SECOND_TRIP, 64), np.arange(SECOND_TRIP, cap)])
    buf, D = free_scene(sb, cap, jittered_grid(6000, 80, (40.0, 40.0), seed=66), seed=67, among=among)
    return _scene("indices past 2^18", buf, 1700.0, D=D)


BIG = {"pile 4097 in 5000": pile_4097, "box 16384": box_16384, "32 cells per side": lambda sb: scan_edge(sb, 32),
       "64 cells per side": lambda sb: scan_edge(sb, 64), "crowd 600": crowd_600}
# scenes that reach the second trip of the loop over the block sums (more than SCAN_SUMS blocks): tests of their own
PAST = {"544 cells per side": cells_544, "indices past 2^18": indices_past_2_18}
_cache = {}


def big_scene(sb, name):
    if name not in _cache:
        _cache[name] = (BIG[name] if name in BIG else PAST[name])(sb)
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


def pairs_above(scene):
    """(above [np], total): per data index up to the highest in use the pairs listed under it (its partners of a larger data
    index) -- the words of the 64-bit scan that places the pair list -- from the reference's whole list"""
    total = int(expected(scene, None, 0, key="plain")[2][0])
    pairs = expected(scene, None, total, key="all")[1]
    return np.bincount(pairs[:, 0], minlength=int(scene["D"].max()) + 1), total


def cut_of(scene):
    """a max_pairs that truncates the list: half way through the pairs listed under data indices from SECOND_TRIP on where the
    scene has such (the cut then lies behind the carry of the scan over the data indices), else half of the list"""
    above, total = pairs_above(scene)
    first = int(above[:SECOND_TRIP].sum())
    return first + (total - first) // 2 if first < total else total // 2


_ref_cache = {}


def expected(scene, labels=None, max_pairs=0, other_body=False, key=None):
    """contacts_ref of the scene as uploaded, computed once per (scene, key) and shared; the arrays are not to be written to"""
    k = (scene["name"], key, max_pairs, other_body)
    if key is None or k not in _ref_cache:
        out = cref.contacts_ref(scene["buf"], scene["radius"], scene["bounds"], labels, max_pairs, other_body, prune=scene.get("prune", False))
        for a in out:
            a.setflags(write=False)
        if key is None:
            return out
        _ref_cache[k] = out
    return _ref_cache[k]
