"""Engine.forces() on this build against the parent commit's only route to the same numbers, load_buffers of all four buffers
(the read-back is a lower bound on that route: the host restatement comes on top).

    python tools/forces_timing.py --parent-tree DIR [--repeats 15] [--out profiles/forces_timing.json]

DIR is a second worktree of the PARENT commit, built.  The protocol is DESIGN.md 5.20's: each build runs in processes of its own,
alternating, three per build, each under its own time limit; a case's figure is the median of the three processes' medians (each a
median of --repeats warm calls), its spread their max - min.  All times are WALL time of the call plus sync().  Scenes: bench config 2
after 64 substeps; config 3 settled (scenes.CONFIG3_SETTLE_FRAMES frames).  This build: forces() into preallocated tensors, all four
outputs, without labels and with labels=True, other_body=True; the first call after an upload with "forces_table_build_us".  The
parent: load_buffers of metadata, mapping, particles and beams.
The bar, per scene: forces() is faster than the parent's load_buffers by more than that read-back's own spread."""
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


def config2_stepped(sb):
    eng, buf = config2(sb)
    eng.step(64)
    return eng, buf


SHAPES = {"config2": config2_stepped, "config3": config3}


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
        r = {"particles": buf.particle_count, "beams": buf.beam_count}
        tpl = buf.copy()
        r["load_buffers"] = timed(eng, a.repeats, a.warmup, lambda: eng.load_buffers(tpl))
        if not a.tree:   # this build
            dev, maxP, maxB = torch.device("cuda", 0), buf.max_particles, buf.max_beams
            rows, beam = torch.empty((maxP, 8), dtype=torch.float32, device=dev), torch.empty((maxP, 2), dtype=torch.int32, device=dev)
            tension, counts = torch.empty(maxB, dtype=torch.float32, device=dev), torch.empty(4, dtype=torch.int64, device=dev)
            plain = lambda: eng.forces(rows=rows, beam_i32=beam, tension=tension, counts=counts)
            now = eng.load_buffers(buf.copy())
            eng.write_buffers(now)
            r["first_forces"] = {"median_ms": once(eng, plain), "table_build_us": eng.info("forces_table_build_us")}
            r["forces"] = timed(eng, a.repeats, a.warmup, plain)
            r["forces_other_body"] = timed(eng, a.repeats, a.warmup, lambda: eng.forces(labels=True, other_body=True, rows=rows, beam_i32=beam,
                                                                                       tension=tension, counts=counts))
            r["forces_beams_only"] = timed(eng, a.repeats, a.warmup, lambda: eng.forces(rows=None, beam_i32=beam, tension=tension))
            r["counts"] = [int(x) for x in counts.cpu()]
            r["cells_per_side"] = eng.info("forces_cells_per_side")
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
                               capture_output=True, text=True, timeout=600)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit("worker %s failed (%d):\n%s" % (label, p.returncode, p.stderr[-2000:]))   # (nothing more is started)
            runs[label].append(json.loads(line[0][7:]))
            print(label, k, {s: {c: round(v["median_ms"], 4) for c, v in r.items() if isinstance(v, dict)} for s, r in runs[label][-1].items()}, flush=True)

    def fold(label, shape, case):
        m = [r[shape][case]["median_ms"] for r in runs[label]]
        return {"medians_ms": m, "ms": statistics.median(m), "spread_ms": max(m) - min(m)}

    res = {"protocol": "wall time of the call + sync(), median of %d warm calls (first_forces: one call after a fresh upload); three such "
                       "figures per case and build, builds alternating, one process each" % a.repeats,
           "bar": "forces() on this build is faster than load_buffers on the parent by more than the spread of the parent's load_buffers",
           "shapes": {}}
    for shape in SHAPES:
        first = runs["this"][0][shape]
        parent = fold("parent", shape, "load_buffers")
        cases = {c: fold("this", shape, c) for c in ("forces", "forces_other_body", "forces_beams_only", "first_forces", "load_buffers")}
        cases["first_forces"]["table_build_us"] = [r[shape]["first_forces"]["table_build_us"] for r in runs["this"]]
        res["shapes"][shape] = {"particles": first["particles"], "beams": first["beams"], "cells_per_side": first["cells_per_side"],
                                "counts": first["counts"], "parent_load_buffers": parent, "this": cases,
                                "bar_met": cases["forces"]["ms"] + parent["spread_ms"] < parent["ms"]}
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
