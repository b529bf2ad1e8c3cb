"""What the tools/batch_*_timing.py tools share: the three scenes their shapes are made of and the wall-clock timing loop."""
import statistics
import time

import numpy as np


def scene(sb, kind, layout, maxp, maxb):
    """kind "default": the default scene (119 / 299); "lattice": a lattice of 32 x 32 (1024 / 2945); "path": a path of maxp
    particles whose data indices, slots and beam slots are shuffled -- the deepest component the capacity allows."""
    if kind == "default":
        return sb.scenes.default_buffers(layout, maxp, maxb)
    buf = sb.Buffers(layout, maxp, maxb)
    if kind == "lattice":
        src = sb.scenes.lattice_buffers(32, 32, d=25.0, origin=(100.0, 100.0), spring=50.0, damp=700.0, yield_strain=0.2, strain_limit=0.5,
                                        jitter=2.0, layout=layout)
        P, B = src.particle_count, src.beam_count
        buf.set_scene(src.particles[:P], src.beams[:B].copy())
        buf.metadata[12:28] = src.metadata[12:28]
        return buf
    # the path: particle k at data index D[k] in slot S[k], beam k (k -- k + 1) at data index E[k] in slot T[k]
    n, rng = maxp, np.random.default_rng(1)
    D, S, E, T = rng.permutation(maxp)[:n], rng.permutation(n), rng.permutation(maxb)[:n - 1], rng.permutation(n - 1)
    buf.particles[D, 0] = 20.0 + 30.0 * (D % 32)
    buf.particles[D, 1] = 20.0 + 30.0 * (D // 32)
    buf.mapping[S] = D
    rec = buf.beams[E]
    rec["a"], rec["b"] = D[:-1], D[1:]
    for f, v in (("length", 30.0), ("target_length", 30.0), ("last_length", 30.0), ("spring", 50.0), ("damp", 700.0),
                 ("yield_strain", 0.2), ("strain_break_limit", 0.5)):
        rec[f] = v
    buf.beams[E] = rec
    buf.mapping[maxp + T] = E
    buf.particle_count, buf.beam_count = n, n - 1
    return buf


def timed(sync, repeats, warmup, call):
    """WALL time of call() plus sync(), warm: the median, the extremes and the count of `repeats` samples behind `warmup`."""
    ms = []
    for k in range(warmup + repeats):
        sync()
        t = time.perf_counter()
        call()
        sync()
        if k >= warmup:
            ms.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}
