"""Scenes, programs and references of the pose tests (sb_batch_pose_device).  The stepped cases and the graphs are
tests/batch_body_summary_cases.py's, imported; what is new here is a scene from bare positions, the caller's references with NaN
rows, and the turned lattice of the geometric property with its bounds.  tests/test_batch_pose_cpu.py runs the oracle side alone
and pins the figures, tests/test_gpu_batch_pose.py runs both sides."""
import numpy as np

import batch_body_summary_cases as qc
import batch_summary_cases as sc

NONFINITE_SCENE = sc.NONFINITE_SCENE


def stepped_cases(sb):
    """The default scene at 120 / 300 after 2 frames, the thrown lattices after 2 frames and mid-frame, the scene with non-finite
    particles at 8 / 8."""
    return [qc.case_default_120_300(sb), qc.case_break(sb), qc.case_saturation(sb)]


def scene_of(sb, pos, vel=None, cap=(8, 8), layout=2):
    """A scene of free particles at `pos` [n, 2] with velocities `vel` (None: at rest), identity mapping, no beams."""
    pts = np.zeros((len(pos), 6), "f4")
    pts[:, 0:2] = pos
    if vel is not None:
        pts[:, 2:4] = vel
    buf = sb.Buffers(layout, *cap)
    buf.set_scene(pts, np.zeros(0, sb.layout.BEAM_DTYPE[layout]))
    return buf


def caller_refs(bufs, maxP, seed=21):
    """One reference array [maxP, 2] float32 per scene of the caller's own: the scene's positions turned by 0.3 about (500, 500)
    and rounded, with about a tenth of the rows NaN (those particles have no reference) and, at data indices that hold no particle,
    values that must never be read into a sum."""
    rng = np.random.default_rng(seed)
    c, s = np.cos(0.3), np.sin(0.3)
    out = []
    for b in bufs:
        ref = np.full((maxP, 2), 12345.0, np.float32)
        if b is not None:
            d = b.mapping[:b.particle_count].astype(np.int64)
            p = b.particles[d, 0:2].astype(np.float64) - 500.0
            ref[d] = np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1]], axis=1) + 500.0
            lost = d[rng.random(len(d)) < 0.1]
            ref[lost, rng.integers(0, 2, len(lost))] = np.nan     # (one NaN float is enough)
        out.append(ref)
    return out


# ---------------------------------------------------------------- the geometric property
THETA = 0.7
RMS_BOUND = 2e-5   # |delta| from the input rounding plus at most 3e-6 from the cancellation I + I0 - 2 sqrt(a^2 + b^2), times two


def turned_lattice(sb, cap=(65, 64)):
    """An 8 x 8 lattice of spacing 4 at integer reference coordinates inside [32, 128)^2; the current positions are that lattice
    turned by THETA about its centroid and shifted, computed in float64 and rounded to float32.  Every coordinate stays below 128,
    so rounding moves it by at most half an ulp of 128, 2^-18, and a position by |delta| <= sqrt(2) 2^-18 = 5.4e-6.  theta_bound is
    2 (|delta| / r_rms + 2^-23) with r_rms = sqrt(I0 / n) of the reference."""
    i, j = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    ref = np.stack([40.0 + 4.0 * i.ravel(), 48.0 + 4.0 * j.ravel()], axis=1)
    centre = ref.mean(axis=0)
    c, s = np.cos(THETA), np.sin(THETA)
    p = ref - centre
    exact = np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1]], axis=1) + centre + np.array([20.0, 10.0])
    now = exact.astype(np.float32)
    assert ref.min() >= 32 and ref.max() < 128 and now.min() >= 32 and now.max() < 128
    delta = np.sqrt(2.0) * 2.0 ** -18
    assert np.hypot(*(now.astype(np.float64) - exact).T).max() <= delta
    r_rms = float(np.sqrt((p * p).sum() / len(p)))
    full = np.full((cap[0], 2), np.nan, np.float32)
    full[:64] = ref
    return dict(buf=scene_of(sb, now, None, cap), ref=full, cap=cap, r_rms=r_rms, delta=delta, theta_bound=2.0 * (delta / r_rms + 2.0 ** -23))
