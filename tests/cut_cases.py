"""Cases of the cut tests (tests/test_cut_cpu.py, tests/test_gpu_cut.py, tests/test_gpu_batch_cut.py).

TABLE: single shape against single beam, (name, shape, A, B, expected).  Rows whose numbers are small integers and halves are
exact in float32 and are also checked against cut_ref's fractions; `expected` is what the header's predicate says.
Scene cases: name -> shapes for a scene; every one must hit something and miss something in the reference (checked on the CPU)."""
import numpy as np

from cut_ref import DISC, NONE, SEGMENT, pack

NAN, INF = float("nan"), float("inf")
BELOW3 = float(np.nextafter(np.float32(3.0), np.float32(0.0)))

TABLE = [
    # knife
    ("proper crossing", (SEGMENT, 0, -1, 0, 1), (-1, 0), (1, 0), True),
    ("apart", (SEGMENT, 3, -1, 3, 1), (-1, 0), (1, 0), False),
    ("beam endpoint exactly on the knife", (SEGMENT, 0, -2, 0, 2), (0, 0), (3, 1), True),
    ("beam endpoint on the knife's line, past its end", (SEGMENT, 0, -2, 0, -1), (0, 0), (3, 1), False),
    ("collinear, overlapping", (SEGMENT, 0, 0, 4, 0), (2, 0), (6, 0), True),
    ("collinear, disjoint", (SEGMENT, 0, 0, 1, 0), (2, 0), (6, 0), False),
    ("collinear, touching at one point", (SEGMENT, 0, 0, 2, 0), (2, 0), (6, 0), True),
    ("zero-length knife on the beam", (SEGMENT, 1, 1, 1, 1), (0, 0), (2, 2), True),
    ("zero-length knife off the beam", (SEGMENT, 1, 1.5, 1, 1.5), (0, 0), (2, 2), False),
    ("zero-length beam on the knife", (SEGMENT, 0, 0, 4, 4), (1, 1), (1, 1), True),
    ("zero-length beam off the knife", (SEGMENT, 0, 0, 4, 4), (1, 2), (1, 2), False),
    ("zero-length knife on a zero-length beam", (SEGMENT, 1, 1, 1, 1), (1, 1), (1, 1), True),
    ("knife ending exactly in the beam's interior", (SEGMENT, 1, 3, 1, 0), (0, 0), (2, 0), True),
    ("knife ending half a unit short of the beam", (SEGMENT, 1, 3, 1, 0.5), (0, 0), (2, 0), False),
    # eraser
    ("disc tangent to the beam", (DISC, 2, 3, 3, 0), (0, 0), (4, 0), True),
    ("disc an ulp short of tangent", (DISC, 2, 3, BELOW3, 0), (0, 0), (4, 0), False),
    ("disc over the interior", (DISC, 2, 1, 1.5, 0), (0, 0), (4, 0), True),
    ("disc past endpoint A, reaching it", (DISC, -3, 4, 5, 0), (0, 0), (4, 0), True),
    ("disc past endpoint A, short of it", (DISC, -3, 4, 4.5, 0), (0, 0), (4, 0), False),
    ("disc past endpoint B, reaching it", (DISC, 7, 4, 5, 0), (0, 0), (4, 0), True),
    ("disc past endpoint B, short of it", (DISC, 7, 4, 4.5, 0), (0, 0), (4, 0), False),
    ("radius 0 on an endpoint", (DISC, 4, 0, 0, 0), (0, 0), (4, 0), True),
    ("radius 0 on the interior", (DISC, 2, 0, 0, 0), (0, 0), (4, 0), True),
    ("radius 0 off the beam", (DISC, 2, 0.5, 0, 0), (0, 0), (4, 0), False),
    ("disc on a zero-length beam", (DISC, 1, 1, 1, 0), (1, 2), (1, 2), True),
    ("negative radius", (DISC, 2, 0, -1, 0), (0, 0), (4, 0), False),
    ("kind NONE", (NONE, 0, -1, 0, 1), (-1, 0), (1, 0), False),
]
EXACT = len(TABLE)   # the rows above hold finite numbers that float32 computes exactly
TABLE += [
    ("NaN radius", (DISC, 2, 0, NAN, 0), (0, 0), (4, 0), False),
    ("NaN in a knife", (SEGMENT, NAN, -1, 0, 1), (-1, 0), (1, 0), False),
    ("NaN in a disc's centre", (DISC, 2, NAN, 10, 0), (0, 0), (4, 0), False),
    ("NaN in a beam, knife", (SEGMENT, 0, -1, 0, 1), (-1, NAN), (1, 0), False),
    ("NaN in a beam, disc", (DISC, 0, 0, 10, 0), (NAN, 0), (1, 0), False),
    # An infinity follows the header's operators like any number (Inf - Inf and 0 * Inf are NaN, the rest compares): what the
    # predicate says is whatever those give, and the reference restates them -- expected None: parity with cut_ref only.
    ("Inf in a beam, knife through its finite end", (SEGMENT, 0, -1, 0, 1), (0, 0), (INF, 0), None),
    ("Inf in a beam, disc over its finite end", (DISC, 0, 0, 1, 0), (0, 0), (INF, 0), None),
    ("Inf in a knife", (SEGMENT, 0, -INF, 0, INF), (-1, 0), (1, 0), None),
    ("infinite radius", (DISC, 2, 1, INF, 0), (0, 0), (4, 0), None),
]


def table_arrays():
    """(shapes uint32 [n, 8], A float32 [n, 2], B float32 [n, 2]) of TABLE"""
    return (pack([c[1] for c in TABLE]), np.asarray([c[2] for c in TABLE], dtype=np.float32),
            np.asarray([c[3] for c in TABLE], dtype=np.float32))


def table_scene(sb, layout=2):
    """TABLE's beams as one scene: beam i joins particles 2 i and 2 i + 1 (a free pair each; nothing steps this scene).  Returns
    (the buffers to upload, with 0 where a coordinate is not finite; the particle records with the table's own coordinates, for
    write_particles_device).  Every shape of TABLE is then tried on every beam of it."""
    n = len(TABLE)
    buf = sb.Buffers(layout, 2 * n + 2, n + 2)
    particles = np.zeros((2 * n, 6), dtype=np.float32)
    beams = np.zeros(n, dtype=buf.beams.dtype)
    for i, c in enumerate(TABLE):
        particles[2 * i, :2], particles[2 * i + 1, :2] = c[2], c[3]
        beams[i]["a"], beams[i]["b"] = 2 * i, 2 * i + 1
    for f in ("length", "target_length", "last_length", "spring", "strain_break_limit"):
        beams[f] = 1.0
    real = particles.copy()
    particles[~np.isfinite(particles)] = 0.0
    buf.set_scene(particles, beams)
    records = np.zeros((buf.max_particles, 6), dtype=np.float32)
    records[:2 * n] = real
    return buf, records


# ---- scene cases: strokes and discs over a scene, by the scene's bounding box (x0, y0, x1, y1) of its particles

def scene_shapes(box):
    x0, y0, x1, y1 = (float(v) for v in box)
    mx, my, w, h = (x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0
    return {
        "vertical stroke": pack([(SEGMENT, mx, y0 - 1, mx, y1 + 1)]),
        "horizontal stroke": pack([(SEGMENT, x0 - 1, my, x1 + 1, my)]),
        "diagonal stroke": pack([(SEGMENT, x0, y0, mx, y1)]),
        "disc": pack([(DISC, mx, my, min(w, h) / 4, 0)]),
        "stroke, none, disc": pack([(SEGMENT, x0 - 1, my + h / 8, mx, my + h / 8), (NONE, 0, 0, 1e9, 1e9), (DISC, x0 + w / 4, y0 + h / 4, min(w, h) / 8, 0)]),
        "64 shapes": pack([(DISC, x0 + w * (i % 8) / 8, y0 + h * (i // 8) / 8, min(w, h) / 40, 0) if i % 2 else
                           (SEGMENT, x0 + w * (i % 8) / 8, y0 + h * (i // 8) / 8, x0 + w * (i % 8 + 0.4) / 8, y0 + h * (i // 8 + 0.3) / 8)
                           for i in range(64)]),
    }


def box_of(buf):
    p = buf.particles[buf.mapping[:buf.particle_count].astype(np.int64), :2]
    return float(p[:, 0].min()), float(p[:, 1].min()), float(p[:, 0].max()), float(p[:, 1].max())


# ---- the engine's scenes (tests/test_gpu_cut.py): name -> make(sb) -> (buffers, bounds)

def lattice(sb, layout=2):
    """test_gpu_reupload.py's breaking lattice: 40 x 30 particles thrown into the corner -- it yields and breaks beams of its own;
    1200 particles are two tiles of the blocked plan and five of a 256-particle tiling"""
    return sb.scenes.lattice_buffers(40, 30, d=30.0, origin=(30.0, 30.0), spring=50.0, damp=100.0, yield_strain=0.05, strain_limit=0.12,
                                     layout=layout, velocity=(-40.0, -35.0), slack=8, jitter=0.5), 4000.0


SCENES = {
    "lattice": lattice,
    "default": lambda sb: (sb.scenes.default_buffers(2, 256, 512), 1000.0),
}


# ---- the batch's scenes (tests/test_gpu_batch_cut.py)

BATCH_CAP = (1024, 4096)
BATCH_K = 3


def full_scene(sb, layout=2):
    """1024 particles / 4096 beams, the capacity of a batch scene: a 32 x 32 lattice with both diagonals (3906 beams) and 190
    beams to the second neighbour in y"""
    p, b = sb.scenes.rectangle(40.0, 40.0, 28.0, 32, 32, 50.0, 300.0, 0.2, 0.6, layout=layout)
    extra = np.zeros(BATCH_CAP[1] - len(b), dtype=b.dtype)
    idx = np.arange(len(extra)) * 5
    idx = idx[(idx % 32) < 30]
    extra = extra[:len(idx)]
    extra["a"], extra["b"] = idx, idx + 2
    for f, v in (("length", 56.0), ("target_length", 56.0), ("last_length", 56.0), ("spring", 50.0), ("damp", 300.0), ("yield_strain", 0.2),
                 ("strain_break_limit", 0.6)):
        extra[f] = v
    more = np.zeros(BATCH_CAP[1] - len(b) - len(extra), dtype=b.dtype)   # what is still missing: second neighbours in x
    j = np.arange(len(more)) * 3
    more["a"], more["b"] = j, j + 64
    for f, v in (("length", 56.0), ("target_length", 56.0), ("last_length", 56.0), ("spring", 50.0), ("damp", 300.0), ("yield_strain", 0.2),
                 ("strain_break_limit", 0.6)):
        more[f] = v
    beams = np.concatenate([b, extra, more])
    assert len(p) == BATCH_CAP[0] and len(beams) == BATCH_CAP[1] and beams["b"].max() < len(p)
    pv = np.zeros((len(p), 6), dtype=np.float32)
    pv[:, :2] = p
    pv[:, 2:4] = (3.0, -6.0)
    buf = sb.Buffers(layout, *BATCH_CAP)
    buf.set_scene(pv, beams)
    return buf


def batch_scenes(sb, layout=2):
    """(buffers per scene -- None: never uploaded --, shapes uint32 [12, BATCH_K, 8]): lattices of different sizes with a different
    stroke each, the full scene, the default scene, two scenes with only NONE shapes, one never uploaded"""
    def lat(w, h, v):
        b = sb.scenes.lattice_buffers(w, h, d=30.0, origin=(60.0, 60.0), spring=50.0, damp=300.0, yield_strain=0.1, strain_limit=0.4, layout=layout,
                                      velocity=v, jitter=0.5, seed=w * h)
        out = sb.Buffers(layout, *BATCH_CAP)
        n = b.particle_count
        out.set_scene(b.particles[:n], b.beams[:b.beam_count])
        return out

    default = sb.Buffers(layout, *BATCH_CAP)
    dp, db = sb.scenes.default_scene(layout)
    default.set_scene(dp, db)
    bufs = [lat(5, 4, (2.0, -3.0)), lat(9, 7, (-4.0, -2.0)), full_scene(sb, layout), None, lat(16, 12, (5.0, -9.0)), default, lat(3, 3, (0.0, -1.0)),
            lat(20, 20, (-6.0, -6.0)), lat(12, 9, (1.0, -8.0)), lat(7, 7, (3.0, 3.0)), lat(30, 4, (0.0, -12.0)), lat(2, 2, (1.0, 1.0))]
    names = ["vertical stroke", "horizontal stroke", "stroke, none, disc", None, "diagonal stroke", "disc", None, "stroke, none, disc",
             "vertical stroke", None, "horizontal stroke", "disc"]
    shapes = np.zeros((len(bufs), BATCH_K, 8), dtype=np.uint32)
    for i, (b, n) in enumerate(zip(bufs, names)):
        if n is not None:   # (the never-uploaded scene gets shapes too: they must do nothing)
            sh = scene_shapes(box_of(b if b is not None else bufs[0]))[n]
            shapes[i, :len(sh)] = sh
    shapes[3] = shapes[0]
    return bufs, shapes
