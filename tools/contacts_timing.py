"""Engine.contacts() against the only route the parent commit offers to the same answer.

    python tools/contacts_timing.py --parent-tree DIR [--repeats 15] [--out profiles/contacts_timing.json]

DIR is a second worktree of the PARENT commit, built.  The protocol is DESIGN.md 5.19's: each build runs in processes of its own,
alternating, three per build; a case's figure is the median of the three processes' medians (each a median of --repeats), its
spread their max - min.  All times are WALL time of the call plus sync(), warm.  Shapes:
  config2      bench config 2's scene: a 1000 x 1000 lattice, 1 M particles / 3 M beams, layout v2, bounds 32000, collisions off,
               after 64 substeps: nothing touches
  config3      bench config 3: scenes.config3_buffers(), the blob pile, spatial-hash collisions, settled CONFIG3_SETTLE_FRAMES frames
  this build   contacts() into preallocated tensors: touch and counts; and the same with a pair list of 1 M rows
  the parent   load_buffers of all four buffers: its read-back ALONE, a lower bound of its route -- the grid on the host that has
               to follow only adds to it
The bar: this build is faster than the parent's read-back by more than the parent's spread, in both shapes, with and without the
pair list.  Reported, not gated: one substep and one frame() of the same scene, bodies(), contacts(labels=True), the first call
after an upload (it builds the table) and the host time of that build, the four count words, the cells per side."""
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
WARM_SUBSTEPS = 64
LIST_ROWS = 1 << 20


def make_engine(sb, shape):
    if shape == "config2":
        eng, buf = config2(sb)
        eng.step(WARM_SUBSTEPS)
    else:
        eng, buf = config3(sb)
    eng.sync()
    return eng, buf


def worker(a):
    import torch
    parent = bool(a.tree)
    sb = load_tree(a.tree) if parent else __import__("__graft_entry__").load_package()
    dev = torch.device("cuda", 0)
    out = {}
    for shape in SHAPES:
        eng, buf = make_engine(sb, shape)
        maxP = buf.max_particles
        r = {"particles": buf.particle_count, "beams": buf.beam_count, "capacity": [maxP, buf.max_beams]}
        back = buf.copy()
        r["load_buffers"] = timed(eng, a.repeats, a.warmup, lambda: eng.load_buffers(back))
        if not parent:
            touch = torch.empty((maxP, 4), dtype=torch.int32, device=dev)
            pairs = torch.empty((LIST_ROWS, 2), dtype=torch.int32, device=dev)
            counts = torch.empty(4, dtype=torch.int64, device=dev)
            labels = torch.empty(maxP, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            eng.sync()
            t = time.perf_counter()
            eng.contacts(touch=touch, counts=counts)
            eng.sync()
            r["first_call_ms"] = (time.perf_counter() - t) * 1e3
            r["table_build_us"] = eng.info("contacts_table_build_us")
            r["cells_per_side"] = eng.info("contacts_cells_per_side")
            r["contacts"] = timed(eng, a.repeats, a.warmup, lambda: eng.contacts(touch=touch, counts=counts))
            r["contacts_list"] = timed(eng, a.repeats, a.warmup, lambda: eng.contacts(touch=touch, counts=counts, pairs=LIST_ROWS, out=pairs))
            r["counts"] = counts.cpu().tolist()
            r["bodies"] = timed(eng, a.repeats, a.warmup, lambda: eng.bodies(labels, False, False))
            r["contacts_labels_true"] = timed(eng, a.repeats, a.warmup, lambda: eng.contacts(labels=True, touch=touch, counts=counts))
        # (the stepping last: it moves the scene on)
        r["substep"] = timed(eng, a.repeats, a.warmup, lambda: eng.step(1))
        r["frame"] = timed(eng, max(3, a.repeats // 3), 1, eng.frame)
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
                       "process each" % a.repeats,
           "parent_route": "load_buffers of all four buffers: the read-back alone, without the grid on the host that has to follow",
           "shapes": {}}
    for shape in SHAPES:
        first = runs["this"][0][shape]
        t, tl, p = fold("this", shape, "contacts"), fold("this", shape, "contacts_list"), fold("parent", shape, "load_buffers")
        res["shapes"][shape] = {
            "particles": first["particles"], "beams": first["beams"], "capacity": first["capacity"], "counts": first["counts"],
            "cells_per_side": first["cells_per_side"], "list_rows": LIST_ROWS,
            "contacts": t, "contacts_list": tl, "parent_load_buffers": p, "this_load_buffers": fold("this", shape, "load_buffers"),
            "speedup": p["ms"] / t["ms"], "speedup_list": p["ms"] / tl["ms"],
            "bar_met": t["ms"] < p["ms"] - p["spread_ms"] and tl["ms"] < p["ms"] - p["spread_ms"],
            "substep": {"this": fold("this", shape, "substep"), "parent": fold("parent", shape, "substep")},
            "frame": {"this": fold("this", shape, "frame"), "parent": fold("parent", shape, "frame")},
            "bodies": fold("this", shape, "bodies"), "contacts_labels_true": fold("this", shape, "contacts_labels_true"),
            "first_call_ms": [r[shape]["first_call_ms"] for r in runs["this"]],
            "table_build_us": [r[shape]["table_build_us"] for r in runs["this"]]}
    res["bar"] = "contacts(), with and without a pair list of 2^20 rows, < the parent's load_buffers - the parent's spread, in both shapes"
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
