"""BatchEngine.bodies beside summary() and one frame() of the same batch.

    python tools/batch_bodies_timing.py [--repeats 15] [--out profiles/batch_bodies_timing.json]

Three processes, one after the other; a case's figure is the median of the three processes' medians (each a median of
--repeats), its spread their max - min.  All times are WALL time of the call plus sync() plus torch.cuda.synchronize(), warm.
Shapes: 4096 default scenes (119 / 299) at capacity 128 / 320 after 3 frames; 256 lattices of 32 x 32 (1024 / 2945) at capacity
1024 / 4096 after 3 frames; 256 copies of a path of 1024 particles whose data indices, slots and beam slots are shuffled
(capacity 1024 / 4096, not stepped): the deepest component the capacity allows.

  bodies    bodies(labels, counts=counts) into preallocated tensors; bodies_sizes: with the sizes tensor as well
  summary   summary(out) into a preallocated tensor          frame   frame(1)
The frame and summary kernels are the commit before's, so those two are its times.
The condition: bodies() costs less than one frame() of the same batch, in all three shapes.  Its ratio to summary() is reported."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_timing_shapes import scene, timed  # noqa: E402

SHAPES = {"default_4096": (4096, 128, 320, 1, "default"), "lattice_32x32_n256": (256, 1024, 4096, 2, "lattice"),
          "shuffled_path_1024_n256": (256, 1024, 4096, 2, "path")}


def worker(a):
    import torch
    sb = __import__("__graft_entry__").load_package()
    dev = torch.device("cuda", 0)
    out = {}
    for name, (n, maxp, maxb, layout, kind) in SHAPES.items():
        buf = scene(sb, kind, layout, maxp, maxb)
        be = sb.BatchEngine(n_scenes=n, layout=layout, max_particles=maxp, max_beams=maxb)
        be.write_scene(buf)
        if kind != "path":
            be.frame(3)

        def sync():
            be.sync()
            torch.cuda.synchronize()
        labels = torch.empty((n, maxp), dtype=torch.int32, device=dev)
        sizes = torch.empty((n, maxp, 2), dtype=torch.int32, device=dev)
        counts = torch.empty((n, 4), dtype=torch.int32, device=dev)
        rows = torch.empty((n, 24), dtype=torch.float32, device=dev)
        r = {"sync_only": timed(sync, a.repeats, a.warmup, lambda: None),
             "bodies": timed(sync, a.repeats, a.warmup, lambda: be.bodies(labels, counts=counts)),
             "bodies_sizes": timed(sync, a.repeats, a.warmup, lambda: be.bodies(labels, sizes, counts)),
             "summary": timed(sync, a.repeats, a.warmup, lambda: be.summary(rows))}
        sync()
        r["counts_row_0"] = counts[0].tolist()
        r["all_rows_equal"] = bool((counts == counts[0]).all())
        r["frame"] = timed(sync, a.repeats, a.warmup, lambda: be.frame(1))    # (last: it moves the scenes on)
        r["kernel"] = {x: be.info(x) for x in ("bodies_kernel_vgprs", "bodies_kernel_scratch_bytes", "bodies_lds_bytes")}
        r["particles_beams"] = [buf.particle_count, buf.beam_count]
        out[name] = r
        be.destroy()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    runs = []
    for k in range(3):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(a.repeats), "--warmup", str(a.warmup)],
                           capture_output=True, text=True, timeout=600)
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit("worker %d failed (%d):\n%s" % (k, p.returncode, p.stderr[-2000:]))
        runs.append(json.loads(line[0][7:]))
        print(k, {s: {c: round(v["median_ms"], 4) for c, v in r.items() if isinstance(v, dict) and "median_ms" in v} for s, r in runs[-1].items()},
              flush=True)

    def fold(shape, case):
        m = [r[shape][case]["median_ms"] for r in runs]
        return {"medians_ms": m, "ms": statistics.median(m), "spread_ms": max(m) - min(m)}

    res = {"protocol": "wall time of the call + sync() + torch.cuda.synchronize(), warm, median of %d; three such medians per case, one "
                       "process each; default scenes and lattices after 3 frames, the path as uploaded" % a.repeats,
           "shapes": {}}
    for shape, (n, maxp, maxb, layout, kind) in SHAPES.items():
        first = runs[0][shape]
        t = {c: fold(shape, c) for c in ("bodies", "bodies_sizes", "summary", "frame", "sync_only")}
        res["shapes"][shape] = {"n_scenes": n, "capacity": [maxp, maxb], "particles_beams": first["particles_beams"], **first["kernel"],
                                "counts_row_0": first["counts_row_0"], "all_rows_equal": all(r[shape]["all_rows_equal"] for r in runs), **t,
                                "bodies_over_frame": t["bodies"]["ms"] / t["frame"]["ms"],
                                "bodies_over_summary": t["bodies"]["ms"] / t["summary"]["ms"],
                                "condition_met": max(t["bodies"]["medians_ms"]) < min(t["frame"]["medians_ms"])}
    res["condition"] = "bodies() < one frame() of the same batch in all three shapes (every median of the one below every median of the other)"
    res["condition_met"] = all(s["condition_met"] for s in res["shapes"].values())
    import torch
    res = {"device": torch.cuda.get_device_name(0), **res}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
