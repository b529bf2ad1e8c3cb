"""Engine.bodies() against the only route the parent commit offers to the same answer.

    python tools/bodies_timing.py --parent-tree DIR [--repeats 15] [--out profiles/bodies_timing.json]

DIR is a second worktree of the PARENT commit, built.  The protocol is DESIGN.md 5.12's: each build runs in processes of its own,
alternating, three per build; a case's figure is the median of the three processes' medians (each a median of --repeats), its
spread their max - min.  All times are WALL time of the call plus sync(), warm.  Shapes:
  config2      bench config 2: a 1000 x 1000 lattice, 1 M particles / 3 M beams, layout v2, bounds 32000, collisions off, after 64
               substeps: one body
  config2_cut  the same lattice after an upload that keeps the plan and cut 1 % of its beams (at random), then 64 substeps
  this build   bodies() into preallocated tensors (labels, sizes and counts)
  the parent   load_buffers of all four buffers: its read-back ALONE, a lower bound of its route -- the union-find on the host that
               has to follow only adds to it
The bar: this build is faster than the parent's read-back by more than the parent's spread, in both shapes.
Reported, not gated: the ratio to one frame() and to summary(); labels alone and counts alone; the first call after an upload (it
builds the tables) and the host time of that build; the four count words."""
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
from engine_timing_shapes import config2, load_tree, timed  # noqa: E402

SHAPES = ("config2", "config2_cut")
WARM_SUBSTEPS = 64


def without(buf, keep):
    """`buf` with only the beams keep[] of its (identity-mapped) beam slots, renumbered in order"""
    import numpy as np
    out = buf.copy()
    recs = buf.beams[:buf.beam_count][keep]
    n = len(recs)
    out.beams[:n] = recs
    out.mapping[buf.max_particles:buf.max_particles + n] = np.arange(n)
    out.beam_count = n
    return out


def make_engine(sb, shape):
    import numpy as np
    eng, buf = config2(sb)
    if shape == "config2_cut":
        buf = without(buf, np.random.default_rng(1).random(buf.beam_count) >= 0.01)
        eng.write_buffers(buf)
        if eng.info("uploads_edited") != 1:
            sys.exit("the cut upload did not keep the plan")
    return eng, buf


def worker(a):
    import torch
    parent = bool(a.tree)
    sb = load_tree(a.tree) if parent else __import__("__graft_entry__").load_package()
    dev = torch.device("cuda", 0)
    out = {}
    for shape in SHAPES:
        eng, buf = make_engine(sb, shape)
        eng.step(WARM_SUBSTEPS)
        eng.sync()
        maxP = buf.max_particles
        r = {"particles": buf.particle_count, "beams": buf.beam_count, "capacity": [maxP, buf.max_beams]}
        r["frame"] = timed(eng, max(3, a.repeats // 3), 1, eng.frame)
        back = buf.copy()
        r["load_buffers"] = timed(eng, a.repeats, a.warmup, lambda: eng.load_buffers(back))
        if not parent:
            labels = torch.empty(maxP, dtype=torch.int32, device=dev)
            sizes = torch.empty((maxP, 2), dtype=torch.int32, device=dev)
            counts = torch.empty(4, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            eng.sync()
            t = time.perf_counter()
            eng.bodies(labels, sizes, counts)
            eng.sync()
            r["first_call_ms"] = (time.perf_counter() - t) * 1e3
            r["table_build_us"] = eng.info("bodies_table_build_us")
            r["bodies"] = timed(eng, a.repeats, a.warmup, lambda: eng.bodies(labels, sizes, counts))
            r["labels_alone"] = timed(eng, a.repeats, a.warmup, lambda: eng.bodies(labels, False, False))
            r["counts_alone"] = timed(eng, a.repeats, a.warmup, lambda: eng.bodies(False, False, counts))
            row = torch.empty(24, dtype=torch.float32, device=dev)
            r["summary"] = timed(eng, a.repeats, a.warmup, lambda: eng.summary(row))
            r["counts"] = counts.cpu().tolist()
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_tree:
        ap.error("--parent-tree is needed")
    runs = {"parent": [], "this": []}
    for k in range(3):
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

    res = {"protocol": "wall time of the call + sync(), warm, median of %d; three such medians per case and build, builds alternating, one "
                       "process each; after %d substeps" % (a.repeats, WARM_SUBSTEPS),
           "parent_route": "load_buffers of all four buffers: the read-back alone, without the union-find on the host that has to follow",
           "shapes": {}}
    for shape in SHAPES:
        first = runs["this"][0][shape]
        t, p = fold("this", shape, "bodies"), fold("parent", shape, "load_buffers")
        frame, summary = fold("this", shape, "frame"), fold("this", shape, "summary")
        res["shapes"][shape] = {
            "particles": first["particles"], "beams": first["beams"], "capacity": first["capacity"], "counts": first["counts"],
            "bodies": t, "parent_load_buffers": p, "this_load_buffers": fold("this", shape, "load_buffers"),
            "speedup": p["ms"] / t["ms"], "bar_met": t["ms"] < p["ms"] - p["spread_ms"],
            "labels_alone": fold("this", shape, "labels_alone"), "counts_alone": fold("this", shape, "counts_alone"),
            "frame": {"this": frame, "parent": fold("parent", shape, "frame")}, "summary": summary,
            "bodies_over_frame": t["ms"] / frame["ms"], "bodies_over_summary": t["ms"] / summary["ms"],
            "first_call_ms": [r[shape]["first_call_ms"] for r in runs["this"]],
            "table_build_us": [r[shape]["table_build_us"] for r in runs["this"]]}
    res["bar"] = "bodies() < the parent's load_buffers - the parent's spread, in both shapes"
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
