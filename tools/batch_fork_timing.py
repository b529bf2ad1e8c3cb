"""BatchEngine.fork / checkpoint / write_beams_device against what the parent commit offers for the same move.

    python tools/batch_fork_timing.py --parent-tree DIR [--repeats 15] [--out profiles/batch_fork_timing.json]

DIR is a second worktree of the PARENT commit, built.  Each build runs in processes of its own, alternating, three per build; a
case's figure is the median of the three processes' medians (each a median of --repeats), its spread their max - min.  All
times are WALL time of the call(s) plus sync(), warm, on N default scenes (119 particles / 299 beams) after 3 frames:
4096 scenes at capacity 128 / 320 and 256 scenes at capacity 1024 / 4096.

  (a) broadcast of scene 0          this: fork(zeros)                         parent: load_scene(0) + write_scene(buf, 0, N)
  (b) 64 sources onto 64 contiguous this: fork(src[i] = e[i // run])          parent: 64 x (load_scene(e[j]) + write_scene(buf, j * run, run))
      runs of run = N / 64
  (c) full-batch copies             this: checkpoint(None); fork(rotation)     parent: reset(None), the yardstick of a full-batch blob copy
  (d) state import                  this: write_beams_device                   parent: write_particles_device
The bar: (a) and (b) beat the parent's route by more than the parent's spread.  (c) and (d) are reported with the bytes they
move (payload: what changes in the batch, not the staging traffic) and the resulting bytes/s."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"default_4096": (4096, 128, 320, 1), "default_in_capacity_1024_4096_n256": (256, 1024, 4096, 2)}


def load_tree(tree):
    import importlib.util
    spec = importlib.util.spec_from_file_location("sb_entry_of_tree", os.path.join(tree, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def timed(be, repeats, warmup, call):
    ms = []
    for k in range(warmup + repeats):
        be.sync()
        t = time.perf_counter()
        call()
        be.sync()
        if k >= warmup:
            ms.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def worker(a):
    import torch
    parent = bool(a.tree)
    sb = load_tree(a.tree) if parent else __import__("__graft_entry__").load_package()
    out = {}
    for name, (n, maxp, maxb, layout) in SHAPES.items():
        buf = sb.scenes.default_buffers(layout, maxp, maxb)
        be = sb.BatchEngine(n_scenes=n, layout=layout, max_particles=maxp, max_beams=maxb)
        be.write_scene(buf)
        be.frame(3)
        run = n // 64
        e = [j * run + run // 2 for j in range(64)]
        p, b, alive = be.state_tensors()
        r = {}
        # what both builds have comes first, from the same state of the process in both
        r["sync_only"] = timed(be, a.repeats, a.warmup, lambda: None)
        r["c_reset_all"] = timed(be, a.repeats, a.warmup, lambda: be.reset())
        r["d_write_particles_device"] = timed(be, a.repeats, a.warmup, lambda: be.write_particles_device(p))
        if parent:
            tmp = buf.copy()

            def route_a():
                be.load_scene(0, tmp)
                be.write_scene(tmp, 0, n)

            def route_b():
                for j in range(64):
                    be.load_scene(e[j], tmp)
                    be.write_scene(tmp, j * run, run)
            r["a_broadcast"] = timed(be, a.repeats, a.warmup, route_a)
            r["b_64_sources"] = timed(be, max(3, a.repeats // 3), 1, route_b)
        else:
            dev = torch.device("cuda", 0)
            zeros = torch.zeros(n, dtype=torch.int32, device=dev)
            runs = torch.tensor(e, dtype=torch.int32, device=dev).repeat_interleave(run)
            rot = ((torch.arange(n, device=dev) + 1) % n).to(torch.int32)
            r["a_broadcast"] = timed(be, a.repeats, a.warmup, lambda: be.fork(zeros))
            r["b_64_sources"] = timed(be, a.repeats, a.warmup, lambda: be.fork(runs))
            r["c_checkpoint_all"] = timed(be, a.repeats, a.warmup, lambda: be.checkpoint())
            r["c_fork_permutation"] = timed(be, a.repeats, a.warmup, lambda: be.fork(rot))
            r["c_fork_permutation_as_reset"] = timed(be, a.repeats, a.warmup, lambda: be.fork(rot, as_reset=True))
            r["d_write_beams_device"] = timed(be, a.repeats, a.warmup, lambda: be.write_beams_device(b, True, True))
            r["blobs"] = {k: be.info(k) for k in ("constant_blob_bytes", "state_blob_bytes", "fork_staging_bytes")}
        out[name] = r
        be.destroy()
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
                sys.exit("worker %s failed (%d):\n%s" % (label, p.returncode, p.stderr[-2000:]))
            runs[label].append(json.loads(line[0][7:]))
            print(label, k, {s: {c: round(v["median_ms"], 4) for c, v in r.items() if "median_ms" in v} for s, r in runs[label][-1].items()}, flush=True)

    def fold(label, shape, case):
        m = [r[shape][case]["median_ms"] for r in runs[label]]
        return {"medians_ms": m, "ms": statistics.median(m), "spread_ms": max(m) - min(m)}

    res = {"protocol": "wall time of the call(s) + sync(), warm, median of %d (the parent's 64-source route: %d); three such medians per case and "
                       "build, builds alternating, one process each; N default scenes (119 / 299) after 3 frames" % (a.repeats, max(3, a.repeats // 3)),
           "shapes": {}}
    for shape, (n, maxp, maxb, layout) in SHAPES.items():
        blobs = runs["this"][0][shape]["blobs"]
        cst, st = blobs["constant_blob_bytes"], blobs["state_blob_bytes"]
        s = {"n_scenes": n, "capacity": [maxp, maxb], **blobs}
        for case in ("a_broadcast", "b_64_sources"):
            t, p = fold("this", shape, case), fold("parent", shape, case)
            s[case] = {"this": t, "parent": p, "speedup": p["ms"] / t["ms"], "bar_met": t["ms"] < p["ms"] - p["spread_ms"]}
        moved = {"c_reset_all": n * st, "c_checkpoint_all": n * st, "c_fork_permutation": n * (cst + 2 * st), "c_fork_permutation_as_reset": n * (cst + 2 * st),
                 "d_write_beams_device": n * 299 * 8, "d_write_particles_device": n * 119 * 24}
        for case, nbytes in moved.items():
            t = fold("this", shape, case)
            s[case] = {"this": t, "payload_bytes": nbytes, "payload_gb_per_s": nbytes / (t["ms"] * 1e-3) / 1e9}
            if case in ("c_reset_all", "d_write_particles_device"):
                s[case]["parent"] = fold("parent", shape, case)
        s["sync_only"] = {"this": fold("this", shape, "sync_only"), "parent": fold("parent", shape, "sync_only")}
        per_byte = lambda c: s[c]["this"]["ms"] / s[c]["payload_bytes"]  # noqa: E731
        s["fork_permutation_cost_per_byte_over_parent_reset"] = per_byte("c_fork_permutation") / (s["c_reset_all"]["parent"]["ms"] / (n * st))
        res["shapes"][shape] = s
    res["bar"] = "(a) and (b): this < parent - parent's spread, in both shapes"
    res["bar_met"] = all(s[c]["bar_met"] for s in res["shapes"].values() for c in ("a_broadcast", "b_64_sources"))
    import torch
    res = {"device": torch.cuda.get_device_name(0), **res}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
