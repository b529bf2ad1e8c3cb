"""The engine's four whole-scene reports on this build against the parent commit: the refactor that gave them one
set of scene tables, one scan and one buffer owner changes no launch, so no call may be slower.

    python tools/engine_reports_timing.py --parent-tree DIR [--repeats 15] [--out profiles/engine_reports_timing.json]

DIR is a second worktree of the PARENT commit, built.  The protocol is DESIGN.md 5.12's: each build runs in processes of its own,
alternating, three per build; a case's figure is the median of the three processes' medians (each a median of --repeats), its
spread their max - min.  All times are WALL time of the call plus sync().  Shapes: bench configs 2 and 3.  Cases, each warm into
preallocated tensors: summary(), bodies(sizes=True), contacts(pairs=1 << 20), body_summary(rows=8) with the engine's labels and
with the caller's.  Also the FIRST call of each report after an upload (it builds the tables: one process-median of one call per
fresh upload), and the first calls of all four in a row after one upload.
The bar, per warm call and per first call of a report on its own: this build's median is not slower than the parent's by more
than the parent's spread.  The four in a row are reported, not gated (one inversion of the particle table replaces four)."""
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

SHAPES = {"config2": config2, "config3": config3}
CASES = ("summary", "bodies", "contacts", "body_summary", "body_summary_labels")
LIST_ROWS = 1 << 20


def calls(eng, buf, torch):
    dev, maxP = torch.device("cuda", 0), buf.max_particles
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
    row, labels, sizes, touch, pairs, rank = torch.empty(24, dtype=torch.float32, device=dev), i32(maxP), i32(maxP, 2), i32(maxP, 4), i32(LIST_ROWS, 2), i32(maxP)
    rows, own = torch.empty((8, 24), dtype=torch.float32, device=dev), (torch.arange(maxP, dtype=torch.int32, device=dev) % 5)
    c4, c8 = i64(4), i64(8)
    return {"summary": lambda: eng.summary(row, c8),
            "bodies": lambda: eng.bodies(labels, sizes, c4),
            "contacts": lambda: eng.contacts(pairs=pairs, touch=touch, counts=c4),
            "body_summary": lambda: eng.body_summary(None, rows=8, out=rows),
            "body_summary_labels": lambda: eng.body_summary(own, rows=8, out=rows)}


def once(eng, call):
    eng.sync()
    t = time.perf_counter()
    call()
    eng.sync()
    return (time.perf_counter() - t) * 1e3


def worker(a):
    import torch
    sb = load_tree(a.tree) if a.tree else __import__("__graft_entry__").load_package()
    out = {}
    for shape, make in SHAPES.items():
        eng, buf = make(sb)
        eng.sync()
        cs = calls(eng, buf, torch)
        r = {"particles": buf.particle_count, "beams": buf.beam_count}
        now = eng.load_buffers(buf.copy())
        for name in CASES:   # a fresh upload of the scene as it is, then the report's first call
            eng.write_buffers(now)
            r["first_" + name] = {"median_ms": once(eng, cs[name])}
        eng.write_buffers(now)
        r["first_all_four"] = {"median_ms": sum(once(eng, cs[name]) for name in CASES[:4])}
        for name in CASES:
            r[name] = timed(eng, a.repeats, a.warmup, cs[name])
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
            print(label, k, {s: {c: round(v["median_ms"], 4) for c, v in r.items() if isinstance(v, dict)} for s, r in runs[label][-1].items()}, flush=True)

    def fold(label, shape, case):
        m = [r[shape][case]["median_ms"] for r in runs[label]]
        return {"medians_ms": m, "ms": statistics.median(m), "spread_ms": max(m) - min(m)}

    res = {"protocol": "wall time of the call + sync(), median of %d warm calls (first_*: one call after a fresh upload); three such figures "
                       "per case and build, builds alternating, one process each" % a.repeats,
           "bar": "this build's median <= the parent's median + the parent's spread, per warm call and per first call of one report",
           "shapes": {}}
    for shape in SHAPES:
        first = runs["this"][0][shape]
        cases = {}
        for case in CASES + tuple("first_" + c for c in CASES) + ("first_all_four",):
            t, p = fold("this", shape, case), fold("parent", shape, case)
            cases[case] = {"this": t, "parent": p, "ratio": t["ms"] / p["ms"]}
            if case != "first_all_four":
                cases[case]["bar_met"] = t["ms"] <= p["ms"] + p["spread_ms"]
        res["shapes"][shape] = {"particles": first["particles"], "beams": first["beams"], "cases": cases}
    res["bar_met"] = all(c.get("bar_met", True) for s in res["shapes"].values() for c in s["cases"].values())
    import torch
    res = {"device": torch.cuda.get_device_name(0), **res}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
