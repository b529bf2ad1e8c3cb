"""Hand-built render scenes, shared by the CPU tests (tests/test_render_ref_cpu.py and tests/test_render_cases_cpu.py: render_ref against
host/render.js, its two beam routes against each other, every case against what its name says) and the GPU tests
(tests/test_gpu_render_edges.py, tests/test_gpu_batch_render_edges.py: sb_render and sb_batch_render_device against render_ref).

A Case states its scene (buffers(sbp, layout)), the pictures it is drawn at (renders: (resolution, bounds_size, particle_radius)),
and what it is built to hit (expect), which tests/test_render_cases_cpu.py asserts from render_ref's own numbers:
  boxes    {particle slot: pixels of the clipped box}
  points   {beam slot: points inside the image}
  ties     [(particle slot, px, py, "r" | "r08")]: the pixel centre is at d == r / d == r * 0.8 of that disc, bit for bit
  first    {beam slot: a lower bound of the first inside k}
  n        {beam slot: (lo, hi)}: lo <= n < hi
  undrawn  beam slots that put no pixel (render.js would not terminate, or the beam misses the image)
Positions are float32: every coordinate here is rounded to float32 when the buffers are made, and every claim is checked on the
loaded buffers.  Where bounds_size == resolution, toPx(v) == v exactly.
"""
import numpy as np

TWO32, TWO52, TWO53 = 2.0 ** 32, 2.0 ** 52, 2.0 ** 53
NAN, INF = float("nan"), float("inf")


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


def reversed_slots(buf):
    """The same records drawn in the opposite slot order."""
    rev = buf.copy()
    P, B, maxP = buf.particle_count, buf.beam_count, buf.max_particles
    rev.mapping[:P] = buf.mapping[:P][::-1]
    rev.mapping[maxP:maxP + B] = buf.mapping[maxP:maxP + B][::-1]
    return rev


def refit(sbp, buf, max_particles, max_beams):
    """`buf` (any mapping) in Buffers of a larger capacity: records keep their data indices, slots their order."""
    out = sbp.Buffers(buf.layout, max_particles, max_beams)
    P, B = buf.particle_count, buf.beam_count
    out.particles[:buf.max_particles] = buf.particles
    out.beams[:buf.max_beams] = buf.beams
    out.mapping[:P] = buf.mapping[:P]
    out.mapping[max_particles:max_particles + B] = buf.mapping[buf.max_particles:buf.max_particles + B]
    out.particle_count, out.beam_count = P, B
    return out


def benign(buf):
    """`buf` with every particle on a lattice inside (0, 1000)^2: what is uploaded before far-off or non-finite positions are
    written on the device."""
    out = buf.copy()
    i = np.arange(buf.max_particles)
    out.particles[:, 0] = 100.0 + 40.0 * (i % 20)
    out.particles[:, 1] = 100.0 + 40.0 * (i // 20 % 20)
    return out


class Case:
    def __init__(self, name, build, renders, layouts=(1, 2), device_positions=False, node=True, nothing=False, expect=None,
                 gpu_renders=None):
        self.name, self._build, self.renders, self.layouts = name, build, renders, layouts
        self.device_positions = device_positions   # the positions cannot be uploaded: the GPU tests import them on the device
        self.node = node                           # render.js can walk it in a few seconds
        self.nothing = nothing                     # the picture is black
        self.expect = expect or {}
        self.gpu_renders = gpu_renders or renders

    def buffers(self, sbp, layout=None):
        return self._build(sbp, self.layouts[0] if layout is None else layout)

    def __repr__(self):
        return self.name


def _pairs(n):
    return [(2 * i, 2 * i + 1) for i in range(n)]


# ---------------------------------------------------------------- the scenes render_ref was first checked on

def _edges(sbp, layout):
    pts = [(-5.0, 500.0), (1005.0, 500.0), (500.0, -4.0), (500.0, 1006.0), (2.0, 3.0), (998.0, 997.0), (-8.0, 1007.0), (1009.0, -9.0),
           (-300.0, 200.0), (1300.0, 800.0), (200.0, -400.0), (800.0, 1500.0), (-50.0, -70.0), (1100.0, 1200.0), (400.0, 400.0),
           (-2000.0, 500.5), (3000.0, 499.5)]
    bms = [(8, 9, 0.1, 0.3), (10, 11, -0.2, -0.4), (12, 13, 0.5, 0.9), (14, 8, 0.0, 0.0), (14, 11, 1.5, -1.5), (15, 16, 0.25, 0.25),
           (0, 1, 0.3, 0.6), (2, 3, 0.7, -0.7), (6, 7, 0.05, 0.1), (9, 8, 0.2, 0.2)]
    return custom(sbp, layout, pts, bms)


def _slot_order(sbp, layout):
    pts = [(500.0, 500.0), (507.0, 503.0), (512.0, 498.0), (100.0, 100.0), (900.0, 900.0), (100.0, 900.0), (900.0, 100.0),
           (300.0, 300.0), (300.0, 700.0)]
    bms = [(3, 4, 0.1, -0.9), (5, 6, 0.6, 0.9), (7, 8, 0.0, 0.3), (8, 7, 0.9, -0.3)]
    return custom(sbp, layout, pts, bms)


NONFINITE_COLOURS = [(NAN, 0.0), (0.0, NAN), (INF, 0.0), (-INF, 0.0), (0.0, INF), (0.0, -INF), (NAN, NAN), (INF, -INF), (1e30, -1e30),
                     (-0.0, -0.0), (0.5, 1e-8), (-3.0, -2.0)]


def _nonfinite_colours(sbp, layout):
    pts = [(100.0 + 80.0 * i, 100.0 + 60.0 * (i % 3)) for i in range(12)] + [(100.0 + 80.0 * i, 800.0) for i in range(12)]
    bms = [(i, 12 + i, sn, ss) for i, (sn, ss) in enumerate(NONFINITE_COLOURS)]
    return custom(sbp, layout, pts, bms)


def _shuffled_mapping(sbp, layout):
    buf = sbp.scenes.default_buffers(layout, 256, 512)
    buf.beams["strain"][:buf.beam_count] = np.linspace(-1.5, 1.5, buf.beam_count, dtype="f4")
    buf.beams["stress"][:buf.beam_count] = np.linspace(1.2, -1.2, buf.beam_count, dtype="f4")
    return shuffled(buf, 9)


# ---------------------------------------------------------------- exact ties (bounds_size == resolution == 64)

def _ties_r5(sbp, layout):
    # offsets of pixel centres from (10.5, 10.5) are integers: 5 = r on the axes and at (3, 4); 4 = 0.8 r on the axes.  The second
    # disc is cut by the corner to 7 x 8 pixels, so its ties are drawn by its own thread
    return custom(sbp, layout, [(10.5, 10.5), (62.5, 1.5)], [])


TIES_R5 = ([(0, 15, 10, "r"), (0, 10, 15, "r"), (0, 5, 10, "r"), (0, 10, 5, "r"), (0, 13, 14, "r"), (0, 14, 13, "r"), (0, 7, 6, "r"),
            (0, 6, 13, "r"), (0, 14, 10, "r08"), (0, 10, 14, "r08"), (0, 6, 10, "r08"), (0, 10, 6, "r08")]
           + [(1, 57, 1, "r"), (1, 62, 6, "r"), (1, 59, 5, "r"), (1, 58, 4, "r"), (1, 58, 1, "r08"), (1, 62, 5, "r08")])


def _ties_r625(sbp, layout):
    # r = 6.25: 0.8 r = 5 at (3, 4) of the first disc; the second's centres are offset by quarters: (3.75, 5) is at 6.25 = r
    return custom(sbp, layout, [(10.5, 10.5), (40.75, 40.5)], [])


TIES_R625 = [(0, 15, 10, "r08"), (0, 13, 14, "r08"), (0, 14, 13, "r08"), (0, 6, 7, "r08"), (0, 7, 14, "r08"),
             (1, 44, 45, "r"), (1, 44, 35, "r")]


# ---------------------------------------------------------------- route thresholds (bounds_size == resolution == 64)

def _discs_r35(sbp, layout):
    # c +- 3.5 is an integer for the .5 centres: floor and ceil return it, the box is 8 x 8 = 64 pixels (a thread draws it); any
    # other centre gives 9 columns or rows (a wave draws it).  Slots 0 / 1 and 2 / 3 overlap, the wide one first and last in turn;
    # slot 4's box ends exactly on the last column and row
    return custom(sbp, layout, [(22.25, 21.3), (20.5, 20.5), (40.5, 40.5), (40.25, 42.5), (59.5, 59.5)], [])


def _discs_r6(sbp, layout):
    # 13-wide boxes (integer centres) cut by an edge to 5 rows: 65 pixels; cut by a corner to 8 x 8: 64, reached only by clipping.
    # Slots 0 / 4 and 1 / 6 overlap, wide under thread and thread under wide
    return custom(sbp, layout, [(60.0, 60.0), (1.0, 1.0), (20.0, -2.0), (40.0, 65.0), (62.0, 62.0), (30.0, 30.0), (3.0, 3.0)], [])


def _beams_32_33(sbp, layout):
    # integer endpoints and a radius below half a pixel diagonal: no disc pixel, x = a + k exactly.  32 and 33 points unclipped,
    # 32 and 33 left by the clip at x = 0, and two verticals of 32 and 33 points crossing all four
    pts = [(10.0, 20.0), (41.0, 20.0), (10.0, 24.0), (42.0, 24.0), (-100.0, 30.0), (31.0, 30.0), (-100.0, 34.0), (32.0, 34.0),
           (20.0, 5.0), (20.0, 36.0), (25.0, 5.0), (25.0, 37.0)]
    cols = [(0.1, -0.9), (0.3, 0.9), (0.6, -0.4), (0.0, 0.4), (0.8, 0.0), (0.45, -0.15)]
    return custom(sbp, layout, pts, [(a, b, sn, ss) for (a, b), (sn, ss) in zip(_pairs(6), cols)])


# ---------------------------------------------------------------- radius extremes

def _radius_huge(sbp, layout):
    return custom(sbp, layout, [(32.0, 32.0), (10.0, 200.0)], [(0, 1, 0.2, 0.5)])


def _radius_tiny(sbp, layout):
    return custom(sbp, layout, [(20.0, 20.0), (40.0, 41.0)], [])


# ---------------------------------------------------------------- far-off beams (bounds_size == resolution == 128, no disc pixel)

def _beyond(c, far, reach):
    """The point `reach` away from c on the line from `far` through c, on the other side of c (float32 places it to ~reach * 2^-24,
    which is what decides where the line crosses the image: `far` alone is too coarse)."""
    c, far = np.asarray(c, np.float64), np.asarray(far, np.float64)
    u = (far - c) / np.hypot(*(far - c))
    return tuple(np.asarray(c - reach * u, np.float32).tolist())


def _far_beams(far, reach, with_ulp_beam):
    F = float(np.float32(far))
    G = float(np.float32(0.3 * far))

    def build(sbp, layout):
        seg = [((40.0, 50.0), (F, G)),                                   # 0: A inside, B far: the first inside k is 0
               ((-F, -0.2 * F), (90.0, 30.0)),                           # 1: A far, B inside: a large first k
               (_beyond((100.0, 10.0), (F, G), reach), (F, G)),          # 2: shallow, (+, +): in through the bottom, out at the right
               ((-F, G), _beyond((30.0, 10.0), (-F, G), reach)),         # 3: shallow, (+, -), A far
               ((G, -F), _beyond((3.0, 100.0), (G, -F), reach)),        # 4: steep, (-, +), A far
               (_beyond((110.0, 40.0), (-G, -F), reach), (-G, -F)),      # 5: steep, (-, -)
               ((-F, 37.0), (reach, 37.0)),                              # 6: dy == 0 on row 37
               ((77.0, F), (77.0, -reach)),                              # 7: dx == 0 on column 77
               (_beyond((120.0, 4.0), (F, F), reach), (F, F)),           # 8: cuts the bottom right corner: a dozen points
               ((-F, F), _beyond((125.0, 125.0), (-F, F), reach))]       # 9: cuts the top right corner: five points, A far
        if with_ulp_beam:
            seg.append(((-(TWO53 - 2.0 ** 29), 10.0), (50.0, 60.0)))     # 10: 2^52 <= n < 2^53: the points step by the ulp
        pts = [p for s in seg for p in s]
        cols = [(0.1 * i - 0.5, 0.17 * i - 0.8) for i in range(len(seg))]
        return custom(sbp, layout, pts, [(a, b, sn, ss) for (a, b), (sn, ss) in zip(_pairs(len(seg)), cols)])
    return build


def _far_miss(far, reach):
    F = float(np.float32(far))

    def build(sbp, layout):
        # slope -1 just outside the corners (0, 0) and (127, 127): x is inside only where y is not
        seg = [((-F, F), _beyond((-1.5, -1.5), (-F, F), reach)), (_beyond((128.5, 128.5), (F, -F), reach), (F, -F))]
        pts = [p for s in seg for p in s]
        return custom(sbp, layout, pts, [(0, 1, 0.1, 0.2), (2, 3, 0.3, -0.2)])
    return build


def _far_n_2p53(sbp, layout):
    # n >= 2^53 (render.js's k++ stops counting): nothing, although B is inside; and the coarser 1e30
    pts = [(-TWO53, 10.0), (50.0, 60.0), (1e30, 20.0), (70.0, 80.0), (30.0, -1e30)]
    return custom(sbp, layout, pts, [(0, 1, 0.1, 0.2), (2, 3, 0.3, -0.2), (3, 4, 0.0, 0.0)])


# ---------------------------------------------------------------- non-finite and far particles (bounds 1000, radius 10, at 64^2)

BIG_PX = TWO53 * 1000.0 / 64.0   # the coordinate whose pixel coordinate is 2^53 at resolution 64


def _nonfinite_particles(sbp, layout):
    pts = [(500.0, 500.0), (NAN, 300.0), (300.0, NAN), (INF, 400.0), (600.0, -INF), (1e30, 500.0), (500.0, -1e30), (1004.0, 480.0),
           (1500.0, -300.0), (BIG_PX * 1.01, 500.0), (BIG_PX * 0.99, 450.0), (200.0, 200.0), (800.0, 250.0), (-6.0, 700.0)]
    ends = [(0, 1), (0, 2), (0, 3), (4, 0), (0, 5), (6, 0), (0, 7), (8, 0), (0, 9), (0, 10), (10, 11), (11, 12), (1, 3), (13, 12)]
    return custom(sbp, layout, pts, [(a, b, 0.07 * i - 0.4, 0.11 * i - 0.7) for i, (a, b) in enumerate(ends)])


def _case_list():
    far = dict(device_positions=True, node=False)
    return [
        Case("edges", _edges, [(128, 1000.0, 10.0), (97, 1000.0, 33.0)]),
        Case("slot_order", _slot_order, [(200, 1000.0, 10.0)]),
        Case("slot_order_reversed", lambda sbp, layout: reversed_slots(_slot_order(sbp, layout)), [(200, 1000.0, 10.0)]),
        Case("nonfinite_colours", _nonfinite_colours, [(160, 1000.0, 10.0)]),
        Case("shuffled_mapping", _shuffled_mapping, [(400, 1000.0, 10.0)], gpu_renders=[(200, 1000.0, 10.0)]),
        Case("ties_r5", _ties_r5, [(64, 64.0, 5.0)], expect=dict(ties=TIES_R5, boxes={0: 144, 1: 56})),
        Case("ties_r625", _ties_r625, [(64, 64.0, 6.25)], expect=dict(ties=TIES_R625)),
        Case("discs_64_65_r35", _discs_r35, [(64, 64.0, 3.5)], expect=dict(boxes={0: 81, 1: 64, 2: 64, 3: 72, 4: 64})),
        Case("discs_64_65_r35_reversed", lambda sbp, layout: reversed_slots(_discs_r35(sbp, layout)), [(64, 64.0, 3.5)],
             expect=dict(boxes={4: 81, 3: 64, 2: 64, 1: 72, 0: 64})),
        Case("discs_64_65_r6", _discs_r6, [(64, 64.0, 6.0)], expect=dict(boxes={0: 100, 1: 64, 2: 65, 3: 65, 4: 64, 5: 169, 6: 100})),
        Case("beams_32_33", _beams_32_33, [(64, 64.0, 0.3)], expect=dict(points={0: 32, 1: 33, 2: 32, 3: 33, 4: 32, 5: 33})),
        Case("beams_32_33_reversed", lambda sbp, layout: reversed_slots(_beams_32_33(sbp, layout)), [(64, 64.0, 0.3)],
             expect=dict(points={5: 32, 4: 33, 3: 32, 2: 33, 1: 32, 0: 33})),
        Case("radius_huge", _radius_huge, [(64, 64.0, 50.0)], expect=dict(boxes={0: 64 * 64})),
        Case("radius_tiny", _radius_tiny, [(64, 64.0, 0.3)], nothing=True, expect=dict(boxes={0: 9, 1: 9})),
        Case("far_beams", _far_beams(1e15, 3e5, True), [(128, 128.0, 0.3)], **far,
             expect=dict(first={1: TWO32, 3: TWO32, 4: TWO32, 9: TWO32, 10: TWO32}, n={10: (TWO52, TWO53)})),
        Case("far_beams_twin", _far_beams(5e6, 3e4, False), [(128, 128.0, 0.3)]),
        Case("far_miss", _far_miss(1e15, 3e5), [(128, 128.0, 0.3)], nothing=True, **far, expect=dict(undrawn=[0, 1])),
        Case("far_miss_twin", _far_miss(5e6, 3e4), [(128, 128.0, 0.3)], nothing=True, expect=dict(undrawn=[0, 1])),
        Case("far_n_2p53", _far_n_2p53, [(128, 128.0, 0.3)], nothing=True, **far,
             expect=dict(undrawn=[0, 1, 2], n={0: (TWO53, INF)})),
        Case("nonfinite_particles", _nonfinite_particles, [(64, 1000.0, 10.0)], **far,
             expect=dict(undrawn=[0, 1, 2, 3, 4, 5, 8, 12], n={8: (TWO53, INF), 9: (TWO52, TWO53), 10: (TWO52, TWO53)},
                         first={10: TWO32})),
    ]


CASES = {c.name: c for c in _case_list()}
UPLOADED = [c.name for c in CASES.values() if not c.device_positions]      # ordinary coordinates: write_buffers carries them
IMPORTED = [c.name for c in CASES.values() if c.device_positions]          # far-off / non-finite positions: written on the device
