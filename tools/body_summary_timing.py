"""Engine.body_summary() against the only bit-reproducible route the parent commit offers to the same answer.

    python tools/body_summary_timing.py --parent-tree DIR [--repeats 15] [--out profiles/body_summary_timing.json]

DIR is a second worktree of the PARENT commit, built.  The protocol is DESIGN.md 5.12's: each build runs in processes of its own,
alternating, three per build, one GPU process at a time; a case's figure is the median of the three processes' medians (each a
median of --repeats), its spread their max - min.  All times are WALL time of the call plus sync(), warm.  Shapes:
  config2      bench config 2's scene: a 1000 x 1000 lattice, 1 M particles / 3 M beams, layout v2, collisions off, after 64
               substeps: ONE body
  config3      bench config 3: scenes.config3_buffers(), the blob pile, spatial-hash collisions, settled: many bodies
  config2cut   config 2 after an upload that removed 1 % of its beams and kept the plan (no delete pass has run)
  this build   body_summary(labels given, rows=8) into preallocated tensors; and bodies() into the labels followed by it
  the parent   load_buffers of all four buffers: its read-back ALONE, a lower bound of its route -- the tree on the host that has
               to follow only adds to it
The bar: both are faster than the parent's read-back by more than the parent's spread, on all three shapes.  Reported, not gated:
the torch route (bodies() + state_tensors() + float64 index_add_; not pinned), one frame(), one summary(), the first call after
an upload with its table build, the call with rank alone and with rows alone, the scratch bytes, the first row's counts."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from engine_timing_shapes import config2, config3, load_tree, timed  # noqa: E402

SHAPES = ("config2", "config3", "config2cut")
WARM_SUBSTEPS = 64
ROWS = 8


def without_a_hundredth(buf):
    """`buf` without every hundredth of its beam slots, renumbered in order (what an editor's cut leaves)"""
    out = buf.copy()
    B, maxP = buf.beam_count, buf.max_particles
    keep = np.arange(B) % 100 != 37
    recs = buf.beams[buf.mapping[maxP:maxP + B].astype(np.int64)][keep]
    n = len(recs)
    out.beams[:n] = recs
    out.mapping[maxP:maxP + n] = np.arange(n)
    out.beam_count = n
    return out


def make_engine(sb, shape):
    if shape in ("config2", "config2cut"):
        eng, buf = config2(sb)
        if shape == "config2cut":
            buf = without_a_hundredth(buf)
            eng.write_buffers(buf)
            assert eng.info("uploads_edited") == 1, "the upload did not keep the plan"
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
    for shape in a.shapes.split(","):
        print("worker: building %s" % shape, file=sys.stderr, flush=True)   # (a sign of life: building a scene takes minutes)
        eng, buf = make_engine(sb, shape)
        print("worker: timing %s" % shape, file=sys.stderr, flush=True)
        maxP = buf.max_particles
        r = {"particles": buf.particle_count, "beams": buf.beam_count, "capacity": [maxP, buf.max_beams]}
        back = buf.copy()
        r["load_buffers"] = timed(eng, a.repeats, a.warmup, lambda: eng.load_buffers(back))
        labels = torch.empty(maxP, dtype=torch.int32, device=dev)

        def torch_route():
            eng.bodies(labels, False, False)
            st = eng.state_tensors()["particles"]
            live = labels >= 0
            acc = torch.zeros((maxP, 6), dtype=torch.float64, device=dev)
            acc.index_add_(0, labels[live].long(), st[live].double())
            torch.cuda.synchronize()

        r["torch_route"] = timed(eng, a.repeats, a.warmup, torch_route)
        if not parent:
            rows = torch.empty((ROWS, 24), dtype=torch.float32, device=dev)
            counts = torch.empty((ROWS, 8), dtype=torch.int64, device=dev)
            rank = torch.empty(maxP, dtype=torch.int32, device=dev)
            eng.bodies(labels, False, False)
            torch.cuda.synchronize()
            eng.sync()
            t = time.perf_counter()
            eng.body_summary(labels, rows=ROWS, out=rows)
            eng.sync()
            r["first_call_ms"] = (time.perf_counter() - t) * 1e3
            r["table_build_us"] = eng.info("body_summary_table_build_us")
            r["body_summary"] = timed(eng, a.repeats, a.warmup, lambda: eng.body_summary(labels, rows=ROWS, out=rows))

            def both():
                eng.bodies(labels, False, False)
                eng.body_summary(labels, rows=ROWS, out=rows)

            r["bodies_and_body_summary"] = timed(eng, a.repeats, a.warmup, both)
            r["bodies"] = timed(eng, a.repeats, a.warmup, lambda: eng.bodies(labels, False, False))
            r["rank_alone"] = timed(eng, a.repeats, a.warmup, lambda: eng.body_summary(labels, rows=ROWS, out=False, rank=rank))
            r["rows_counts_rank"] = timed(eng, a.repeats, a.warmup, lambda: eng.body_summary(labels, rows=ROWS, out=rows, counts=counts, rank=rank))
            r["own_labels"] = timed(eng, a.repeats, a.warmup, lambda: eng.body_summary(None, rows=ROWS, out=rows))
            r["first_rows_counts"] = counts.cpu().tolist()[:3]
            r["bodies_in_scene"] = int(rank.max().item()) + 1
            r["scratch_bytes"] = eng.info("body_summary_scratch_bytes")
        summary_row = torch.empty(24, dtype=torch.float32, device=dev)
        r["summary"] = timed(eng, a.repeats, a.warmup, lambda: eng.summary(out=summary_row))
        # (the stepping last: it moves the scene on)
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
    ap.add_argument("--shapes", default=",".join(SHAPES), help="a subset, comma separated: a run of all three takes over twenty minutes")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_tree:
        ap.error("--parent-tree is needed")
    runs = {"parent": [], "this": []}
    for k in range(3):
        for label, extra in (("parent", ["--tree", a.parent_tree]), ("this", [])):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(a.repeats), "--warmup", str(a.warmup), "--shapes", a.shapes] + extra,
                               stdout=subprocess.PIPE, text=True, timeout=1500)   # (the worker's stderr passes through)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit("worker %s failed (%d)" % (label, p.returncode))
            runs[label].append(json.loads(line[0][7:]))
            print(label, k, {s: {c: round(v["median_ms"], 4) for c, v in r.items() if isinstance(v, dict) and "median_ms" in v}
                             for s, r in runs[label][-1].items()}, flush=True)

    def fold(label, shape, case):
        m = [r[shape][case]["median_ms"] for r in runs[label]]
        return {"medians_ms": m, "ms": statistics.median(m), "spread_ms": max(m) - min(m)}

    res = {"protocol": "wall time of the call + sync(), warm, median of %d; three such medians per case and build, builds alternating, one "
                       "GPU process at a time" % a.repeats,
           "parent_route": "load_buffers of all four buffers: the read-back alone, without the tree on the host that has to follow",
           "rows": ROWS, "shapes": {}}
    for shape in a.shapes.split(","):
        first = runs["this"][0][shape]
        t, tb, p = fold("this", shape, "body_summary"), fold("this", shape, "bodies_and_body_summary"), fold("parent", shape, "load_buffers")
        res["shapes"][shape] = {
            "particles": first["particles"], "beams": first["beams"], "capacity": first["capacity"], "bodies_in_scene": first["bodies_in_scene"],
            "first_rows_counts": first["first_rows_counts"], "scratch_bytes": first["scratch_bytes"],
            "body_summary": t, "bodies_and_body_summary": tb, "parent_load_buffers": p, "this_load_buffers": fold("this", shape, "load_buffers"),
            "speedup": p["ms"] / t["ms"], "speedup_with_bodies": p["ms"] / tb["ms"],
            "bar_met": t["ms"] < p["ms"] - p["spread_ms"] and tb["ms"] < p["ms"] - p["spread_ms"],
            "not_gated": {"torch_route": {"this": fold("this", shape, "torch_route"), "parent": fold("parent", shape, "torch_route")},
                          "frame": {"this": fold("this", shape, "frame"), "parent": fold("parent", shape, "frame")},
                          "summary": {"this": fold("this", shape, "summary"), "parent": fold("parent", shape, "summary")},
                          "bodies": fold("this", shape, "bodies"), "rank_alone": fold("this", shape, "rank_alone"),
                          "rows_counts_rank": fold("this", shape, "rows_counts_rank"), "own_labels": fold("this", shape, "own_labels"),
                          "first_call_ms": [r[shape]["first_call_ms"] for r in runs["this"]],
                          "table_build_us": [r[shape]["table_build_us"] for r in runs["this"]]}}
    res["bar"] = ("body_summary(labels given, rows=8), and bodies() + body_summary together, < the parent's load_buffers - the parent's "
                  "spread, on all three shapes")
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
