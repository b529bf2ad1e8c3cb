"""BatchEngine.summary against what the parent commit offers for the same numbers.

    python tools/batch_summary_timing.py --parent-tree DIR [--repeats 15] [--out profiles/batch_summary_timing.json]

DIR is a second worktree of the PARENT commit, built.  Each build runs in processes of its own, alternating, three per build; a
case's figure is the median of the three processes' medians (each a median of --repeats), its spread their max - min.  All
times are WALL time of the call(s) plus sync() plus torch.cuda.synchronize(), warm.  Shapes: 4096 default scenes (119 / 299) at
capacity 128 / 320 and 256 lattices of 32 x 32 (1024 / 2945) at capacity 1024 / 4096, each after 3 frames.

  summary   this: summary(out) into a preallocated [N, 24] tensor
            parent: read_state_device into preallocated tensors (filled with NaN / False once, outside the clock), then the torch
            reductions of parent_route() below into a preallocated [N, 24] tensor: the row's 20 meaningful columns in float32.
            Words 3 (pending break flags) and 20 (uploaded) are not in the parent's export; its route writes 0 there.
The bar: in both shapes summary() beats the parent's route by more than the parent's spread.
Reported, not gated: the bytes each route moves, and on this build rollout(inputs [16, N, 8]) with summaries against a Python
loop of 16 x (write_user_input(device), frame(), summary(out[t]))."""
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

SHAPES = {"default_4096": (4096, 128, 320, 1, "default"), "lattice_32x32_n256": (256, 1024, 4096, 2, "lattice")}
ROLLOUT_T = 16


def load_tree(tree):
    import importlib.util
    spec = importlib.util.spec_from_file_location("sb_entry_of_tree", os.path.join(tree, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def parent_route(torch, be, p, b, alive, out):
    """The row from the state export: NaN-aware reductions over [N, maxP, 6], [N, maxB, 4], [N, maxB]."""
    be.read_state_device(p, b, alive)
    nan, inf = float("nan"), float("inf")
    exists = ~torch.isnan(p).all(dim=2)
    fin = torch.isfinite(p).all(dim=2)
    n = fin.sum(dim=1)
    some = n > 0
    pz = torch.where(fin[..., None], p, torch.zeros((), device=p.device))
    mean = pz[:, :, :4].sum(dim=1) / n[:, None]
    v2 = pz[:, :, 2] * pz[:, :, 2] + pz[:, :, 3] * pz[:, :, 3]
    x, y = p[:, :, 0], p[:, :, 1]
    bex = ~torch.isnan(b[:, :, 0])
    bfin = alive & torch.isfinite(b[:, :, 2]) & torch.isfinite(b[:, :, 3])
    nb = bfin.sum(dim=1)
    bsome = nb > 0
    strain, stress = b[:, :, 2], b[:, :, 3]
    zero = torch.zeros_like(mean[:, 0])
    cols = [exists.sum(dim=1).float(), alive.sum(dim=1).float(), (bex & ~alive).sum(dim=1).float(), zero,
            (exists & ~fin).sum(dim=1).float(), (alive & ~bfin).sum(dim=1).float(),
            mean[:, 0], mean[:, 1], mean[:, 2], mean[:, 3],
            torch.where(some, torch.where(fin, x, inf).amin(dim=1), nan), torch.where(some, torch.where(fin, y, inf).amin(dim=1), nan),
            torch.where(some, torch.where(fin, x, -inf).amax(dim=1), nan), torch.where(some, torch.where(fin, y, -inf).amax(dim=1), nan),
            0.5 * v2.sum(dim=1), torch.where(some, v2.amax(dim=1), nan),
            torch.where(bsome, torch.where(bfin, strain, -inf).amax(dim=1), nan), torch.where(bsome, torch.where(bfin, stress, -inf).amax(dim=1), nan),
            torch.where(bsome, torch.where(bfin, stress, inf).amin(dim=1), nan),
            torch.where(bfin, strain, torch.zeros((), device=p.device)).sum(dim=1) / nb, zero, zero, zero, zero]
    torch.stack(cols, dim=1, out=out)


def worker(a):
    import torch
    parent = bool(a.tree)
    sb = load_tree(a.tree) if parent else __import__("__graft_entry__").load_package()
    dev = torch.device("cuda", 0)
    out = {}
    for name, (n, maxp, maxb, layout, kind) in SHAPES.items():
        buf = scene(sb, kind, layout, maxp, maxb)
        be = sb.BatchEngine(n_scenes=n, layout=layout, max_particles=maxp, max_beams=maxb)
        be.write_scene(buf)
        be.frame(3)

        def sync():
            be.sync()
            torch.cuda.synchronize()
        p, b, alive = be.state_tensors()
        rows = torch.empty((n, 24), dtype=torch.float32, device=dev)
        r = {"sync_only": timed(sync, a.repeats, a.warmup, lambda: None),
             "export_route": timed(sync, a.repeats, a.warmup, lambda: parent_route(torch, be, p, b, alive, rows)),
             "export_alone": timed(sync, a.repeats, a.warmup, lambda: be.read_state_device(p, b, alive))}
        sync()
        route_rows = rows.clone()
        if not parent:
            r["summary"] = timed(sync, a.repeats, a.warmup, lambda: be.summary(rows))
            sync()
            # the two routes agree (float32 sums in another order on the export's side: approximately)
            cols = [c for c in range(20) if c != 3]
            close = torch.isclose(rows[:, cols], route_rows[:, cols], rtol=1e-3, atol=1e-4, equal_nan=True)
            r["routes_agree"] = bool(close.all())
            T = ROLLOUT_T
            ins = torch.zeros((T, n, 8), dtype=torch.float32, device=dev)
            ins[:, :, 0] = 1.0
            ins[:, :, 6] = torch.linspace(-0.05, 0.05, n, device=dev)[None, :]
            outs = torch.empty((T, n, 24), dtype=torch.float32, device=dev)

            def loop():
                for t in range(T):
                    be.write_user_input(ins[t])
                    be.frame()
                    be.summary(outs[t])
            k = max(3, a.repeats // 3)
            r["frames_alone_T16"] = timed(sync, k, 1, lambda: be.frame(T))
            r["rollout_T16"] = timed(sync, k, 1, lambda: be.rollout(ins, out=outs))
            r["python_loop_T16"] = timed(sync, k, 1, loop)
            r["kernel"] = {x: be.info(x) for x in ("summary_kernel_vgprs", "summary_kernel_scratch_bytes", "state_blob_bytes")}
        r["counts"] = [buf.particle_count, buf.beam_count]
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
            print(label, k, {s: {c: round(v["median_ms"], 4) for c, v in r.items() if isinstance(v, dict) and "median_ms" in v}
                             for s, r in runs[label][-1].items()}, flush=True)

    def fold(label, shape, case):
        m = [r[shape][case]["median_ms"] for r in runs[label]]
        return {"medians_ms": m, "ms": statistics.median(m), "spread_ms": max(m) - min(m)}

    res = {"protocol": "wall time of the call(s) + sync() + torch.cuda.synchronize(), warm, median of %d (the T = 16 cases: %d); three such "
                       "medians per case and build, builds alternating, one process each; scenes after 3 frames" % (a.repeats, max(3, a.repeats // 3)),
           "shapes": {}}
    for shape, (n, maxp, maxb, layout, kind) in SHAPES.items():
        first = runs["this"][0][shape]
        P, B = first["counts"]
        t, p = fold("this", shape, "summary"), fold("parent", shape, "export_route")
        s = {"n_scenes": n, "capacity": [maxp, maxb], "particles_beams": [P, B], **first["kernel"],
             "summary": {"this": t, "parent_export_route": p, "this_build_export_route": fold("this", shape, "export_route"),
                         "speedup": p["ms"] / t["ms"], "bar_met": t["ms"] < p["ms"] - p["spread_ms"]},
             "routes_agree": all(r[shape]["routes_agree"] for r in runs["this"]),
             "export_alone": {"this": fold("this", shape, "export_alone"), "parent": fold("parent", shape, "export_alone")},
             "sync_only": {"this": fold("this", shape, "sync_only"), "parent": fold("parent", shape, "sync_only")},
             # the export's tensors, which its reductions read at least once, against what k_batch_summary reads (exists / alive bytes
             # of the capacity, the records of the scene's particles and live beams, flag words, metadata) and the rows it writes
             "bytes": {"export_tensors": n * (maxp * 24 + maxb * 17),
                       "summary_read_at_most": n * (maxp + 2 * maxb + P * 24 + B * 16 + (maxb + 31) // 32 * 4 + 128),
                       "summary_written": n * 96}}
        fr, ro, lo = (fold("this", shape, c) for c in ("frames_alone_T16", "rollout_T16", "python_loop_T16"))
        s["rollout_T16"] = {"frames_alone": fr, "rollout": ro, "python_loop": lo, "loop_over_rollout": lo["ms"] / ro["ms"]}
        res["shapes"][shape] = s
    res["bar"] = "summary(): this < parent's export route - parent's spread, in both shapes"
    res["bar_met"] = all(s["summary"]["bar_met"] for s in res["shapes"].values())
    import torch
    res = {"device": torch.cuda.get_device_name(0), **res}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
