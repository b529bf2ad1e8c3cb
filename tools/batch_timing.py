"""BatchEngine against the loop a user writes without it.

    python tools/batch_timing.py [--repeats 25] [--out profiles/batch_timing.json] [--sizes 256,4096,32768]

Everything in one process, warm, median of --repeats, one frame of 64 substeps + the delete pass:
  baseline  ONE sb.Engine on the default scene (119 particles / 299 beams), wall clock per frame() + sync(), for collision_mode
            ALLPAIRS and for the default GRID; the better of the two is t1.  N scenes done that way cost N * t1 (the engines share
            one GPU and each frame is a chain of dependent launches).
  batch     BatchEngine with N scenes of the default scene, collisions on: HIP events on the batch's stream around frame(); tN / N
            per scene-frame.  Also N = 4096 of a 32 x 32 lattice (1024 particles: the O(P^2) walk at the capacity limit) with
            collisions on and off.
The bar: at N = 4096 the batch's time per scene-frame is at most t1 / 32.

    python tools/batch_timing.py --grid --parent-tree DIR [--out profiles/batch_grid_timing.json]

The contact cells of SB_COLLIDE_GRID against a build of the PARENT commit in DIR (a second worktree, built), same protocol, each
build in processes of its own, alternating, three medians per shape and build: the default scene and the 32 x 32 lattice at
N = 4096 and 256, the default scene in a batch of the limit capacity, the pile of tests/batch_grid_cases.py at N = 4096 (reset before every timed frame: it bursts), and a sweep over
replicated lattices of 64 .. 1024 particles with the cells forced on and off (the break-even that becomes the default
grid_min_particles)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def engine_frame_ms(sb, buf, mode, repeats, warmup):
    eng = sb.Engine(layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=mode)
    eng.write_buffers(buf)
    for _ in range(warmup):
        eng.frame()
    eng.sync()
    ms = []
    for _ in range(repeats):
        t = time.perf_counter()
        eng.frame()
        eng.sync()
        ms.append((time.perf_counter() - t) * 1e3)
    eng.destroy()
    return summary(ms)


def batch_frame_ms(sb, torch, buf, n, mode, repeats, warmup):
    be = sb.BatchEngine(n_scenes=n, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=mode)
    be.write_scene(buf)
    stream = torch.cuda.ExternalStream(be.stream(), device=torch.device("cuda", 0))
    for _ in range(warmup):
        be.frame()
    be.sync()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        be.frame()
        e1.record(stream)
        be.sync()
        ms.append(e0.elapsed_time(e1))
    r = summary(ms)
    r.update(n_scenes=n, per_scene_frame_us=r["median_ms"] * 1e3 / n,
             **{k: be.info(k) for k in ("threads_per_scene", "lds_bytes_per_scene", "materials_in_lds", "scenes_per_cu",
                                        "frame_kernel_vgprs", "frame_kernel_scratch_bytes")})
    be.destroy()
    return r


def load_tree(tree):
    """The package of another checkout (the parent's build) under the same module name: one tree per process."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("sb_entry_of_tree", os.path.join(tree, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def grid_shape_ms(sb, torch, buf, n, repeats, warmup, mode=2, grid_min=None, reset=False, has_cells=True):
    kw = {} if grid_min is None else {"grid_min_particles": grid_min}
    be = sb.BatchEngine(n_scenes=n, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=mode, **kw)
    be.write_scene(buf)
    stream = torch.cuda.ExternalStream(be.stream(), device=torch.device("cuda", 0))
    ms = []
    for k in range(warmup + repeats):
        if reset:
            be.reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        be.frame()
        e1.record(stream)
        be.sync()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    r = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms), "scenes_per_cu": be.info("scenes_per_cu"),
         "lds_bytes_per_scene": be.info("lds_bytes_per_scene")}
    if has_cells:                                                # (the parent's build has no such keys)
        r.update(cells_per_side=be.info("contact_cells_per_side"), cell_substeps=be.info("cell_substeps"),
                 cell_overflow_substeps=be.info("cell_overflow_substeps"), grid_min_particles=be.info("grid_min_particles"))
    be.destroy()
    return r


def grid_shapes(sb):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import batch_grid_cases as gc
    lat = sb.scenes.lattice_buffers(32, 32, d=25.0, origin=(100.0, 100.0), strain_limit=0.5, jitter=2.0, layout=2)
    big = sb.Buffers(2, 1024, 4096)
    big.set_scene(lat.particles[:1024], lat.beams[:lat.beam_count].copy())
    shapes = {"default_4096": (sb.scenes.default_buffers(1, 128, 320), 4096, {}), "default_256": (sb.scenes.default_buffers(1, 128, 320), 256, {}),
              "lattice32_4096": (big, 4096, {}), "lattice32_256": (big, 256, {}), "lattice32_4096_collisions_off": (big, 4096, {"mode": 0}),
              "pile_4096": (gc.pile_buffers(sb), 4096, {"reset": True}),
              # small scenes in a batch of the limit capacity: the cells' kernel and LDS with every scene on the walk
              "default_in_capacity_1024_4096_n256": (sb.scenes.default_buffers(2, 1024, 4096), 256, {})}
    sweep = {}
    for w, h in ((8, 8), (16, 8), (16, 16), (32, 16), (32, 32)):
        src = sb.scenes.lattice_buffers(w, h, d=25.0, origin=(100.0, 100.0), strain_limit=0.5, jitter=2.0, layout=2)
        buf = sb.Buffers(2, w * h, (src.beam_count + 63) // 64 * 64)
        buf.set_scene(src.particles[:w * h], src.beams[:src.beam_count].copy())
        sweep[w * h] = buf
    return shapes, sweep


def grid_worker(a):
    import torch
    sb = load_tree(a.tree) if a.tree else __import__("__graft_entry__").load_package()
    shapes, sweep = grid_shapes(sb)
    out = {}
    for name, (buf, n, kw) in shapes.items():
        slow = name.startswith("lattice32_4096") and a.tree and not name.endswith("off")
        out[name] = grid_shape_ms(sb, torch, buf, n, 7 if slow else a.repeats, 1 if slow else a.warmup, has_cells=not a.tree, **kw)
    if a.sweep:
        out["default_4096_cells_forced"] = grid_shape_ms(sb, torch, shapes["default_4096"][0], 4096, a.repeats, a.warmup, grid_min=1)
        out["default_4096_walk_forced"] = grid_shape_ms(sb, torch, shapes["default_4096"][0], 4096, a.repeats, a.warmup, grid_min=0xFFFFFFFF)
        out["sweep"] = {}
        for P, buf in sweep.items():
            rep = a.repeats if P <= 256 else 7
            out["sweep"][str(P)] = {"cells": grid_shape_ms(sb, torch, buf, 4096, rep, 2, grid_min=1),
                                    "walk": grid_shape_ms(sb, torch, buf, 4096, rep, 2, grid_min=0xFFFFFFFF)}
    print("RESULT " + json.dumps(out), flush=True)


def grid_main(a):
    import subprocess
    runs = {"parent": [], "this": []}
    for k in range(3):
        for label, extra in (("parent", ["--tree", a.parent_tree]), ("this", ["--sweep"] if k == 0 else [])):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--grid-worker", "--repeats", str(a.repeats), "--warmup", str(a.warmup)] + extra,
                               capture_output=True, text=True, timeout=900)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit("worker %s failed (%d):\n%s" % (label, p.returncode, p.stderr[-2000:]))
            runs[label].append(json.loads(line[0][7:]))
            print(label, k, {n: round(v["median_ms"], 4) for n, v in runs[label][-1].items() if "median_ms" in v}, flush=True)
    res = {"protocol": "warm, median of %d (7 for the parent's 32 x 32 lattice with collisions), HIP events on the batch's stream around one frame() "
                       "= 64 substeps + delete pass; three such medians per shape and build, builds alternating, one process each" % a.repeats,
           "shapes": {}}
    for name in runs["parent"][0]:
        pm, tm = [r[name]["median_ms"] for r in runs["parent"]], [r[name]["median_ms"] for r in runs["this"]]
        res["shapes"][name] = {"parent_medians_ms": pm, "this_medians_ms": tm, "parent_ms": statistics.median(pm), "this_ms": statistics.median(tm),
                               "parent_spread_ms": max(pm) - min(pm), "ratio_to_parent": statistics.median(tm) / statistics.median(pm),
                               "this": runs["this"][0][name], "parent": runs["parent"][0][name]}
    off = res["shapes"]["lattice32_4096_collisions_off"]["this_ms"]
    for name in ("lattice32_4096",):
        res["shapes"][name]["ratio_to_no_collisions"] = res["shapes"][name]["this_ms"] / off
        res["shapes"][name]["parent_ratio_to_no_collisions"] = res["shapes"][name]["parent_ms"] / res["shapes"]["lattice32_4096_collisions_off"]["parent_ms"]
    pile = runs["this"][0]["pile_4096"]
    res["pile_overflow_share"] = pile["cell_overflow_substeps"] / max(1, pile["cell_substeps"] + pile["cell_overflow_substeps"])
    first = runs["this"][0]
    res["default_scene_cells_vs_walk_ms"] = {"cells": first["default_4096_cells_forced"], "walk": first["default_4096_walk_forced"]}
    res["sweep_4096_scenes_ms"] = first["sweep"]
    import torch
    res = {"device": torch.cuda.get_device_name(0), **res}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--grid-worker", action="store_true")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="256,4096,32768")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.grid_worker:
        return grid_worker(a)
    if a.grid:
        if not a.parent_tree:
            ap.error("--grid needs --parent-tree")
        return grid_main(a)
    import torch
    import __graft_entry__ as ge
    sb = ge.load_package()
    small = sb.scenes.default_buffers(1, 128, 320)
    res = {"scene": "the reference's default scene, 119 particles / 299 beams, v1, capacity 128 / 320, subticks 64, one frame",
           "engine_allpairs": engine_frame_ms(sb, small, 1, a.repeats, a.warmup),
           "engine_grid": engine_frame_ms(sb, small, 2, a.repeats, a.warmup)}
    t1 = min(res["engine_allpairs"]["median_ms"], res["engine_grid"]["median_ms"])
    res["t1_ms"] = t1
    res["batch"] = []
    for n in [int(x) for x in a.sizes.split(",") if x]:
        r = batch_frame_ms(sb, torch, small, n, 2, a.repeats, a.warmup)
        r["speedup_over_n_engines"] = t1 * 1e3 / r["per_scene_frame_us"]
        res["batch"].append(r)
        print(json.dumps(r), flush=True)
    at4096 = next((r for r in res["batch"] if r["n_scenes"] == 4096), None)
    if at4096:
        res["bar"] = "per scene-frame at N = 4096 <= t1 / 32"
        res["bar_met"] = at4096["per_scene_frame_us"] <= t1 * 1e3 / 32.0
    lat = sb.scenes.lattice_buffers(32, 32, d=25.0, origin=(100.0, 100.0), strain_limit=0.5, jitter=2.0, layout=2)
    big = sb.Buffers(2, 1024, 4096)
    big.set_scene(lat.particles[:1024], lat.beams[:lat.beam_count].copy())
    res["lattice_32x32_collisions_on"] = batch_frame_ms(sb, torch, big, 4096, 2, max(3, a.repeats // 5), 1)
    res["lattice_32x32_collisions_off"] = batch_frame_ms(sb, torch, big, 4096, 0, max(3, a.repeats // 5), 1)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), **res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
