"""BatchEngine.bodies + pose beside one frame() of the same batch on the parent commit and beside the torch route.

    python tools/batch_pose_timing.py [--parent PATH] [--repeats 15] [--out profiles/batch_pose_timing.json]

DESIGN.md 5.12's protocol: three processes, one after the other, each under its own time limit; a case's figure is the median of
the three processes' medians (each a median of --repeats), its spread their max - min.  All times are WALL time of the call(s) plus
sync() plus torch.cuda.synchronize(), warm.  The shapes and scenes are tools/batch_bodies_timing.py's: 4096 default scenes at
128 / 320 after 3 frames; 256 lattices of 32 x 32 at 1024 / 4096 after 3 frames; 256 shuffled paths of 1024 (not stepped).

  label_and_pose    bodies(labels, counts=counts) + pose(labels, rows=8, out=rows, moments=moments), preallocated tensors
  pose              the second call alone, on labels already there
  frame             frame(1), the yardstick.  --parent names a checkout of the PARENT commit with its library built: the frame is
                    then timed there, in processes of its own (three more, alternating with this tree's); without it the frame
                    is this tree's, and the result says so
  torch_route       bodies() + state_tensors() + a float64 index_add_ per scene-and-label of the same eleven sums against the
                    uploaded positions; its sums land in whatever order the atomics take and it cannot see the reset state, so
                    it is not the same answer: reported, not gated
The bar (DESIGN.md 5.14's): labelling and pose together cost less than the parent's frame() of the same batch in all three shapes,
by more than that frame's own spread."""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_bodies_timing as bt  # noqa: E402  (the shapes)
from batch_timing_shapes import scene, timed  # noqa: E402

CASES = ("label_and_pose", "pose", "torch_route", "sync_only")
ROWS = 8


def load_package(root):
    spec = importlib.util.spec_from_file_location("graft_entry_of_" + str(abs(hash(root))), os.path.join(root, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def torch_route(be, ref, torch):
    """The eleven sums per body the way a caller had to take them before: export everything, scatter-add in float64."""
    labels, _ = be.bodies()
    p, _, _ = be.state_tensors()
    n, maxp = labels.shape
    live = labels >= 0
    key = (torch.arange(n, device=labels.device)[:, None] * maxp + labels.clamp(min=0).long())[live]
    x, y, vx, vy = (p[..., k][live].double() for k in range(4))
    rx, ry = ref[..., 0][live].double(), ref[..., 1][live].double()
    leaves = torch.stack([x, y, rx, ry, vx, vy, x * rx + y * ry, rx * y - ry * x, x * x + y * y, rx * rx + ry * ry, x * vy - y * vx], dim=1)
    sums = torch.zeros((n * maxp, 11), dtype=torch.float64, device=labels.device)
    sums.index_add_(0, key, leaves)
    return sums


def worker(a):
    import torch
    sb = load_package(a.root)
    dev = torch.device("cuda", 0)
    out = {}
    for name, (n, maxp, maxb, layout, kind) in bt.SHAPES.items():
        buf = scene(sb, kind, layout, maxp, maxb)
        be = sb.BatchEngine(n_scenes=n, layout=layout, max_particles=maxp, max_beams=maxb)
        be.write_scene(buf)
        uploaded = None if a.frame_only else be.state_tensors()[0][..., :2].contiguous()
        if kind != "path":
            be.frame(3)

        def sync():
            be.sync()
            torch.cuda.synchronize()
        r = {"particles_beams": [buf.particle_count, buf.beam_count]}
        if not a.frame_only:
            labels = torch.empty((n, maxp), dtype=torch.int32, device=dev)
            counts = torch.empty((n, 4), dtype=torch.int32, device=dev)
            rows = torch.empty((n, ROWS, 24), dtype=torch.float32, device=dev)
            moments = torch.empty((n, ROWS, 8), dtype=torch.float64, device=dev)

            def both():
                be.bodies(labels, counts=counts)
                be.pose(labels, rows=ROWS, out=rows, moments=moments)
            r.update({"sync_only": timed(sync, a.repeats, a.warmup, lambda: None),
                      "label_and_pose": timed(sync, a.repeats, a.warmup, both),
                      "pose": timed(sync, a.repeats, a.warmup, lambda: be.pose(labels, rows=ROWS, out=rows, moments=moments)),
                      "torch_route": timed(sync, a.repeats, a.warmup, lambda: torch_route(be, uploaded, torch))})
            sync()
            again = moments.clone()
            both()
            sync()
            r["moments_repeat_bit_for_bit"] = bool(torch.equal(again.view(torch.int64), moments.view(torch.int64)))
            r["row_0_particles"] = rows[0, :, 0].tolist()
            r["kernel"] = {x: be.info(x) for x in ("pose_kernel_vgprs", "pose_kernel_scratch_bytes", "pose_lds_bytes")}
        r["frame"] = timed(sync, a.repeats, a.warmup, lambda: be.frame(1))    # (last: it moves the scenes on)
        out[name] = r
        be.destroy()
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(a, root, frame_only):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
    p = subprocess.run(cmd + (["--frame-only"] if frame_only else []), capture_output=True, text=True, timeout=300)
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.exit("worker on %s failed (%d):\n%s" % (root, p.returncode, p.stderr[-2000:]))
    return json.loads(line[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--frame-only", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: frame() is timed there")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    runs, frames = [], []
    for k in range(3):   # one process at a time, each under its own time limit
        runs.append(run_worker(a, ROOT, False))
        frames.append(run_worker(a, os.path.abspath(a.parent), True) if a.parent else runs[-1])
        print(k, {s: {c: round(r[c]["median_ms"], 4) for c in CASES} for s, r in runs[-1].items()},
              {s: round(r["frame"]["median_ms"], 4) for s, r in frames[-1].items()}, flush=True)

    def fold(rs, shape, case):
        m = [r[shape][case]["median_ms"] for r in rs]
        return {"medians_ms": m, "ms": statistics.median(m), "spread_ms": max(m) - min(m)}

    res = {"protocol": "wall time of the call(s) + sync() + torch.cuda.synchronize(), warm, median of %d; three such medians per case, one "
                       "process each; default scenes and lattices after 3 frames, the path as uploaded; %d rows per scene; ref = the "
                       "reset state (the upload)" % (a.repeats, ROWS),
           "frame_of": "the parent commit, in processes of its own" if a.parent else "THIS tree (no --parent given)", "shapes": {}}
    for shape, (n, maxp, maxb, layout, kind) in bt.SHAPES.items():
        first = runs[0][shape]
        t = {c: fold(runs, shape, c) for c in CASES}
        t["frame"] = fold(frames, shape, "frame")
        t["frame_this_tree"] = fold(runs, shape, "frame")
        res["shapes"][shape] = {"n_scenes": n, "capacity": [maxp, maxb], "particles_beams": first["particles_beams"], **first["kernel"],
                                "row_0_particles": first["row_0_particles"],
                                "moments_repeat_bit_for_bit": all(r[shape]["moments_repeat_bit_for_bit"] for r in runs), **t,
                                "label_and_pose_over_frame": t["label_and_pose"]["ms"] / t["frame"]["ms"],
                                "torch_route_over_label_and_pose": t["torch_route"]["ms"] / t["label_and_pose"]["ms"],
                                "bar_met": max(t["label_and_pose"]["medians_ms"]) < min(t["frame"]["medians_ms"]) - t["frame"]["spread_ms"]}
    res["bar"] = ("bodies() + pose(rows=8, moments=True) < one frame() of the same batch on the parent commit in all three shapes, by "
                  "more than that frame's own spread (every median of the one below every median of the other less the spread)")
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
