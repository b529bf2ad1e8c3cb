"""BatchEngine.bodies + body_summary beside one frame() of the same batch and beside the torch route.

    python tools/batch_body_summary_timing.py [--repeats 15] [--out profiles/batch_body_summary_timing.json]

DESIGN.md 5.12's protocol: three processes, one after the other; a case's figure is the median of the three processes' medians
(each a median of --repeats), its spread their max - min.  All times are WALL time of the call(s) plus sync() plus
torch.cuda.synchronize(), warm.  The shapes and scenes are tools/batch_bodies_timing.py's: 4096 default scenes at 128 / 320
after 3 frames; 256 lattices of 32 x 32 at 1024 / 4096 after 3 frames; 256 shuffled paths of 1024 (not stepped).

  label_and_score   bodies(labels, counts=counts) + body_summary(labels, rows=8, out=rows), preallocated tensors
  body_summary      the second call alone, on labels already there
  frame             frame(1): the commit before's kernel, the yardstick
  torch_route       bodies() + state_tensors() + a float64 index_add_ per scene-and-label for the four means; its sums land in
                    whatever order the atomics take, so it is not bit-pinned: reported, not gated
The condition: labelling and scoring together cost less than one frame() of the same batch, in all three shapes."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_bodies_timing as bt  # noqa: E402  (the shapes)
from batch_timing_shapes import scene, timed  # noqa: E402

CASES = ("label_and_score", "body_summary", "frame", "torch_route", "sync_only")
ROWS = 8


def torch_route(be, torch):
    """The per-body means of x, y, vx, vy the way a caller had to take them before: export everything, scatter-add in float64."""
    labels, _ = be.bodies()
    p, _, _ = be.state_tensors()
    n, maxp = labels.shape
    live = labels >= 0
    key = (torch.arange(n, device=labels.device)[:, None] * maxp + labels.clamp(min=0).long())[live]
    sums = torch.zeros((n * maxp, 4), dtype=torch.float64, device=labels.device)
    sums.index_add_(0, key, p[..., :4][live].double())
    cnt = torch.zeros(n * maxp, dtype=torch.float64, device=labels.device)
    cnt.index_add_(0, key, torch.ones_like(key, dtype=torch.float64))
    return (sums / cnt[:, None]).float()


def worker(a):
    import torch
    sb = __import__("__graft_entry__").load_package()
    dev = torch.device("cuda", 0)
    out = {}
    for name, (n, maxp, maxb, layout, kind) in bt.SHAPES.items():
        buf = scene(sb, kind, layout, maxp, maxb)
        be = sb.BatchEngine(n_scenes=n, layout=layout, max_particles=maxp, max_beams=maxb)
        be.write_scene(buf)
        if kind != "path":
            be.frame(3)

        def sync():
            be.sync()
            torch.cuda.synchronize()
        labels = torch.empty((n, maxp), dtype=torch.int32, device=dev)
        counts = torch.empty((n, 4), dtype=torch.int32, device=dev)
        rows = torch.empty((n, ROWS, 24), dtype=torch.float32, device=dev)

        def both():
            be.bodies(labels, counts=counts)
            be.body_summary(labels, rows=ROWS, out=rows)
        r = {"sync_only": timed(sync, a.repeats, a.warmup, lambda: None),
             "label_and_score": timed(sync, a.repeats, a.warmup, both),
             "body_summary": timed(sync, a.repeats, a.warmup, lambda: be.body_summary(labels, rows=ROWS, out=rows)),
             "torch_route": timed(sync, a.repeats, a.warmup, lambda: torch_route(be, torch))}
        sync()
        again = rows.clone()
        both()
        sync()
        r["rows_repeat_bit_for_bit"] = bool(torch.equal(again.view(torch.int32), rows.view(torch.int32)))
        r["row_0_particles"] = rows[0, :, 0].tolist()
        r["frame"] = timed(sync, a.repeats, a.warmup, lambda: be.frame(1))    # (last: it moves the scenes on)
        r["kernel"] = {x: be.info(x) for x in ("body_summary_kernel_vgprs", "body_summary_kernel_scratch_bytes", "body_summary_lds_bytes")}
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
    for k in range(3):   # one process at a time, each under its own time limit
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(a.repeats), "--warmup", str(a.warmup)],
                           capture_output=True, text=True, timeout=300)
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit("worker %d failed (%d):\n%s" % (k, p.returncode, p.stderr[-2000:]))
        runs.append(json.loads(line[0][7:]))
        print(k, {s: {c: round(r[c]["median_ms"], 4) for c in CASES} for s, r in runs[-1].items()}, flush=True)

    def fold(shape, case):
        m = [r[shape][case]["median_ms"] for r in runs]
        return {"medians_ms": m, "ms": statistics.median(m), "spread_ms": max(m) - min(m)}

    res = {"protocol": "wall time of the call(s) + sync() + torch.cuda.synchronize(), warm, median of %d; three such medians per case, one "
                       "process each; default scenes and lattices after 3 frames, the path as uploaded; %d rows per scene" % (a.repeats, ROWS),
           "shapes": {}}
    for shape, (n, maxp, maxb, layout, kind) in bt.SHAPES.items():
        first = runs[0][shape]
        t = {c: fold(shape, c) for c in CASES}
        res["shapes"][shape] = {"n_scenes": n, "capacity": [maxp, maxb], "particles_beams": first["particles_beams"], **first["kernel"],
                                "row_0_particles": first["row_0_particles"],
                                "rows_repeat_bit_for_bit": all(r[shape]["rows_repeat_bit_for_bit"] for r in runs), **t,
                                "label_and_score_over_frame": t["label_and_score"]["ms"] / t["frame"]["ms"],
                                "torch_route_over_label_and_score": t["torch_route"]["ms"] / t["label_and_score"]["ms"],
                                "condition_met": max(t["label_and_score"]["medians_ms"]) < min(t["frame"]["medians_ms"])}
    res["condition"] = ("bodies() + body_summary(rows=8) < one frame() of the same batch in all three shapes (every median of the one "
                        "below every median of the other)")
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
