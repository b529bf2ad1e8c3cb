"""What the tools/{summary,bodies,contacts,body_summary,engine_reports}_timing.py tools share: loading a second worktree's package,
the engines of bench configs 2 and 3, and the wall-clock timing loop."""
import importlib.util
import os
import statistics
import time


def load_tree(tree):
    """the package of a second worktree (the parent commit, built), through its own __graft_entry__"""
    spec = importlib.util.spec_from_file_location("sb_entry_of_tree", os.path.join(tree, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def config2(sb):
    """bench config 2 uploaded: a 1000 x 1000 lattice, 1 M particles / 3 M beams, layout v2, bounds 32000, collisions off"""
    buf = sb.scenes.lattice_buffers(1000, 1000, d=30.0, origin=(1000.0, 1000.0), jitter=1.0, layout=2)
    eng = sb.Engine(bounds_size=32000.0, layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=0)
    eng.write_buffers(buf)
    return eng, buf


def config3(sb):
    """bench config 3 uploaded and settled: the lattice on the floor under the spatial hash"""
    buf, bounds = sb.scenes.config3_buffers()
    eng = sb.Engine(bounds_size=float(bounds), layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=2)
    eng.write_buffers(buf)
    for _ in range(sb.scenes.CONFIG3_SETTLE_FRAMES):
        eng.frame()
    return eng, buf


def timed(eng, repeats, warmup, call):
    """wall time of call() + sync(), `repeats` times after `warmup` unmeasured ones"""
    ms = []
    for k in range(warmup + repeats):
        eng.sync()
        t = time.perf_counter()
        call()
        eng.sync()
        if k >= warmup:
            ms.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}
