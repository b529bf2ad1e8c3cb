"""Engine.raycast() against the only route the parent commit offers to the same answer.

    python tools/raycast_timing.py --parent-tree DIR [--repeats 15] [--out profiles/raycast_timing.json]

DIR is a second worktree of the PARENT commit, built.  The protocol is DESIGN.md 5.20's: each build runs in processes of its own,
alternating, three per build; a case's figure is the median of the three processes' medians (each a median of --repeats), its
spread their max - min.  All times are WALL time of the call plus sync(), warm.  Shapes:
  config2      bench config 2's scene: a 1000 x 1000 lattice, 1 M particles / 3 M beams, layout v2, bounds 32000, collisions off,
               after 64 substeps
  config3      bench config 3: scenes.config3_buffers(), the blob pile, spatial-hash collisions, settled CONFIG3_SETTLE_FRAMES frames
  this build   raycast() of 64, 4096 and 2^20 rows into preallocated tensors, two ray shapes, two masks: `fan` -- from the centre of
               the particles' box, all directions --, `cross` -- rows along y from x = 0 to x = bounds over the strip above the
               particles (nothing but the far wall is met: no early exit) --; mask 7 (a row with beams walks its whole line) and
               mask 5 (particles and walls: the walk stops early)
  the parent   load_buffers of all four buffers: its read-back ALONE, a lower bound of its route -- the host loop over rays and
               primitives that has to follow only adds to it
The bar: raycast() of 4096 rows is faster than the parent's read-back by more than the parent's spread, both ray shapes (mask 7), both
scenes.  Reported, not gated: the other widths and mask 5, the first call after an upload (table build plus scratch), the count words,
the cells per side, and the sweep's cost: 4096 fan rows after ONE beam has been made long (its endpoint moved across the box with
write_particles_device: counts word 6 says how many)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from engine_timing_shapes import config2, config3, load_tree, timed  # noqa: E402

SHAPES = ("config2", "config3")
WIDTHS = (64, 4096, 1 << 20)
WARM_SUBSTEPS = 64


def make_engine(sb, shape):
    if shape == "config2":
        eng, buf = config2(sb)
        eng.step(WARM_SUBSTEPS)
    else:
        eng, buf = config3(sb)
    eng.sync()
    return eng, buf


def rows_of(sb, torch, box, bounds, shape, n, mask):
    """[n, 8] rows on the device; box: (x0, y0, x1, y1) of the particles"""
    dev = torch.device("cuda", 0)
    k = torch.arange(n, device=dev, dtype=torch.float32)
    if shape == "fan":
        a = k * (6.283185307179586 / n)
        origin = torch.tensor([0.5 * (box[0] + box[2]), 0.5 * (box[1] + box[3])], device=dev).expand(n, 2).contiguous()
        direction = torch.stack([torch.cos(a), torch.sin(a)], 1)
    else:
        y = box[3] + 50.0 + (bounds - box[3] - 100.0) * (k / n)
        origin = torch.stack([torch.zeros_like(y), y], 1)
        direction = torch.tensor([1.0, 0.0], device=dev).expand(n, 2).contiguous()
    return sb.engine.ray_rows(origin.contiguous(), direction, float("inf"), mask=mask)


def worker(a):
    import numpy as np
    import torch
    parent = bool(a.tree)
    sb = load_tree(a.tree) if parent else __import__("__graft_entry__").load_package()
    dev = torch.device("cuda", 0)
    out = {}
    for shape in SHAPES:
        eng, buf = make_engine(sb, shape)
        bounds = 32000.0 if shape == "config2" else float(sb.scenes.config3_buffers()[1])
        r = {"particles": buf.particle_count, "beams": buf.beam_count, "capacity": [buf.max_particles, buf.max_beams]}
        back = buf.copy()
        r["load_buffers"] = timed(eng, a.repeats, a.warmup, lambda: eng.load_buffers(back))
        if not parent:
            pos = back.particles[back.mapping[:back.particle_count].astype(np.int64), :2]
            box = [float(pos[:, 0].min()), float(pos[:, 1].min()), float(pos[:, 0].max()), float(pos[:, 1].max())]
            r["box"] = box
            n_max = max(WIDTHS)
            t = torch.empty(n_max, dtype=torch.float32, device=dev)
            hit = torch.empty((n_max, 3), dtype=torch.int32, device=dev)
            counts = torch.empty(8, dtype=torch.int64, device=dev)
            first = rows_of(sb, torch, box, bounds, "fan", 64, 7)
            torch.cuda.synchronize()
            eng.sync()
            t0 = time.perf_counter()
            eng.raycast(first, t=t, hit=hit, counts=counts)
            eng.sync()
            r["first_call_ms"] = (time.perf_counter() - t0) * 1e3
            r["table_build_us"] = eng.info("raycast_table_build_us")
            r["cells_per_side"] = eng.info("raycast_cells_per_side")
            for rays in ("fan", "cross"):
                for mask in (7, 5):
                    for n in WIDTHS:
                        rows = rows_of(sb, torch, box, bounds, rays, n, mask)
                        torch.cuda.synchronize()
                        key = "%s_mask%d_%d" % (rays, mask, n)
                        r[key] = timed(eng, a.repeats if n < (1 << 20) else max(3, a.repeats // 3), a.warmup if n < (1 << 20) else 1,
                                       lambda: eng.raycast(rows, t=t, hit=hit, counts=counts))
                        r[key]["counts"] = counts.cpu().tolist()
            # the sweep over leftovers: one beam made long
            st = eng.state_tensors()["particles"]
            d = int(back.mapping[0])
            st[d, 0] = bounds - 5.0
            eng.write_particles_device(st)
            rows = rows_of(sb, torch, box, bounds, "fan", 4096, 7)
            r["fan_mask7_4096_with_leftovers"] = timed(eng, a.repeats, a.warmup, lambda: eng.raycast(rows, t=t, hit=hit, counts=counts))
            r["fan_mask7_4096_with_leftovers"]["counts"] = counts.cpu().tolist()
        out[shape] = r
        eng.destroy()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_tree:
        ap.error("--parent-tree is needed")
    runs = {"parent": [], "this": []}
    for k in range(a.processes):
        for label, extra in (("parent", ["--tree", a.parent_tree]), ("this", [])):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(a.repeats), "--warmup", str(a.warmup)] + extra,
                               capture_output=True, text=True, timeout=900)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit("worker %s failed (%d):\n%s" % (label, p.returncode, p.stderr[-2000:]))
            runs[label].append(json.loads(line[0][7:]))
            print(label, k, {s: {c: round(v["median_ms"], 4) for c, v in r.items() if isinstance(v, dict) and "median_ms" in v}
                             for s, r in runs[label][-1].items()}, flush=True)

    def fold(label, shape, case):
        m = [r[shape][case]["median_ms"] for r in runs[label]]
        return {"medians_ms": m, "ms": statistics.median(m), "spread_ms": max(m) - min(m)}

    res = {"protocol": "wall time of the call + sync(), warm, median of %d; %d such medians per case and build, builds alternating, one "
                       "process each" % (a.repeats, a.processes),
           "parent_route": "load_buffers of all four buffers: the read-back alone, without the host loop over rays that has to follow",
           "shapes": {}}
    for shape in SHAPES:
        first = runs["this"][0][shape]
        p = fold("parent", shape, "load_buffers")
        cases = {c: dict(fold("this", shape, c), counts=first[c]["counts"]) for c in first if isinstance(first[c], dict) and "counts" in first[c]}
        gated = ["fan_mask7_4096", "cross_mask7_4096"]
        res["shapes"][shape] = {
            "particles": first["particles"], "beams": first["beams"], "capacity": first["capacity"], "box": first["box"],
            "cells_per_side": first["cells_per_side"], "raycast": cases, "parent_load_buffers": p, "this_load_buffers": fold("this", shape, "load_buffers"),
            "speedup_4096": {c: p["ms"] / cases[c]["ms"] for c in gated},
            "bar_met": all(cases[c]["ms"] < p["ms"] - p["spread_ms"] for c in gated),
            "first_call_ms": [r[shape]["first_call_ms"] for r in runs["this"]],
            "table_build_us": [r[shape]["table_build_us"] for r in runs["this"]]}
    res["bar"] = "raycast() of 4096 rows, fan and cross, mask 7 < the parent's load_buffers - the parent's spread, in both scenes"
    res["bar_met"] = all(s["bar_met"] for s in res["shapes"].values())
    import torch
    res = {"device": torch.cuda.get_device_name(0), **res}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
