"""Engine.summary() against the only route the parent commit offers to the same numbers.

    python tools/summary_timing.py --parent-tree DIR [--repeats 15] [--out profiles/summary_timing.json]
                                   [--stats kernel_stats.csv] [--hbm-calib-gbps X]

DIR is a second worktree of the PARENT commit, built.  The protocol is DESIGN.md 5.12's: each build runs in processes of its own,
alternating, three per build; a case's figure is the median of the three processes' medians (each a median of --repeats), its
spread their max - min.  All times are WALL time of the call(s) plus sync(), warm.  Shapes:
  config2        bench config 2: a 1000 x 1000 lattice, 1 M particles / 3 M beams, layout v2, bounds 32000, collisions off, after
                 64 substeps
  lattice_32x32  a 32 x 32 lattice at capacity 1024 / 4096, collisions off, after 64 substeps
  this build   summary() into preallocated tensors (row and counts)
  the parent   read_state_device into preallocated tensors, then the torch reductions written out in parent_route() below: the
               same 23 numbers except the pending break flags, which no export of the parent reaches (word 3 is left out there);
               its sums are torch's, in whatever order torch reduces
The bar: this build is faster than the parent's route by more than the parent's spread, in both shapes.
Reported, not gated: the bytes each route moves; the default `partials` against one size either side (the default should be the
fastest at 1 M particles); a frame's time with and without a summary behind it; the first call after an upload (it builds the
tables) and the host time of that build; with --stats (the kernel_stats.csv of a separate `rocprofv3 --kernel-trace --stats` run
of `--worker`) the time of the two leaf kernels (pass 1) and their achieved bytes/s, against --hbm-calib-gbps (what
tools/hbm_calib.hip measured on the same device)."""
import argparse
import csv
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

SHAPES = ("config2", "lattice_32x32")
WARM_SUBSTEPS = 64


def make_engine(sb, shape):
    if shape == "config2":
        return config2(sb)
    lat = sb.scenes.lattice_buffers(32, 32, d=25.0, origin=(100.0, 100.0), spring=50.0, damp=700.0, yield_strain=0.2, strain_limit=0.5,
                                    jitter=2.0, layout=2)
    buf = sb.Buffers(2, 1024, 4096)
    buf.set_scene(lat.particles[:lat.particle_count], lat.beams[:lat.beam_count].copy())
    buf.metadata[12:28] = lat.metadata[12:28]
    eng = sb.Engine(bounds_size=1000.0, layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=0)
    eng.write_buffers(buf)
    return eng, buf


def pow2_at_least(n):
    w = 1
    while w < n:
        w *= 2
    return w


def parent_route(eng, torch, tp, tb, ta, out):
    """What a driver of the parent commit does for the same numbers: export, then reduce with torch.  `out`: float64 [24]."""
    eng.read_state_device(tp, tb, ta)
    # (rows of no particle / beam keep the NaN / 0 the tensors were filled with once: never written by the export)
    held = ~torch.isnan(tp).all(dim=1)
    fin = torch.isfinite(tp).all(dim=1)
    f = tp[fin].double()
    n = f.shape[0]
    live = ta != 0
    bfin = live & torch.isfinite(tb[:, 2]) & torch.isfinite(tb[:, 3])
    strain, stress = tb[bfin, 2], tb[bfin, 3]
    v2 = f[:, 2] * f[:, 2] + f[:, 3] * f[:, 3]
    out[0] = held.sum()
    out[1] = live.sum()
    out[2] = (~torch.isnan(tb[:, 0]) & ~live).sum()
    out[4] = held.sum() - n
    out[5] = live.sum() - bfin.sum()
    out[6:10] = f[:, :4].sum(dim=0) / n
    out[10:12] = f[:, :2].amin(dim=0)
    out[12:14] = f[:, :2].amax(dim=0)
    out[14] = 0.5 * v2.sum()
    out[15] = v2.amax()
    out[16] = strain.amax()
    out[17] = stress.amax()
    out[18] = stress.amin()
    out[19] = strain.double().sum() / bfin.sum()
    out[20] = 1.0


def bytes_moved(P, B, maxP, maxB, n1p, n1b):
    """HBM bytes (every array element read or written once)"""
    leaf_p = P * 4 + P * 24 + 5 * n1p * 8                # data index -> particle, pos / vel / acc, 5 partial columns out
    leaf_b = B * 8 + B * (4 + 4 + 4) + B // 8 + n1b * 8  # data index -> {slot, copy}, dead word, strain, stress, flag bits, 1 column out
    folds = 2 * (5 * n1p + n1b) * 8                      # at most: every partial read once and a fraction rewritten
    export = P * (24 + 4 + 24) + B * (8 + 4 + 16 + 16 + 1)  # tools/state_io_timing.py kernel_bytes
    reductions = maxP * 24 * 6 + maxB * 16 * 4 + maxB * 3   # the passes parent_route makes over the exported tensors, at least
    return {"summary_leaf_particles": leaf_p, "summary_leaf_beams": leaf_b, "summary_folds_at_most": folds,
            "summary_total_at_most": leaf_p + leaf_b + folds, "parent_export": export, "parent_torch_reductions_at_least": reductions,
            "parent_total_at_least": export + reductions}


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
        maxP, maxB = buf.max_particles, buf.max_beams
        r = {"particles": buf.particle_count, "beams": buf.beam_count, "capacity": [maxP, maxB]}
        r["sync_only"] = timed(eng, a.repeats, a.warmup, lambda: None)
        r["frame"] = timed(eng, max(3, a.repeats // 3), 1, eng.frame)
        if parent:
            tp = torch.full((maxP, 6), float("nan"), dtype=torch.float32, device=dev)
            tb = torch.full((maxB, 4), float("nan"), dtype=torch.float32, device=dev)
            ta = torch.zeros(maxB, dtype=torch.uint8, device=dev)
            res = torch.zeros(24, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            r["route"] = timed(eng, a.repeats, a.warmup, lambda: parent_route(eng, torch, tp, tb, ta, res))
            r["export_only"] = timed(eng, a.repeats, a.warmup, lambda: eng.read_state_device(tp, tb, ta))
        else:
            row = torch.empty(24, dtype=torch.float32, device=dev)
            counts = torch.empty(8, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            eng.sync()
            t = time.perf_counter()
            eng.summary(row, counts)
            eng.sync()
            r["first_call_ms"] = (time.perf_counter() - t) * 1e3
            r["table_build_us"] = eng.info("summary_table_build_us")
            r["route"] = timed(eng, a.repeats, a.warmup, lambda: eng.summary(row, counts))
            m0 = eng.info("summary_partials")
            r["default_partials"] = m0
            r["partials"] = {str(m): timed(eng, a.repeats, a.warmup, lambda m=m: eng.summary(row, counts, partials=m))
                             for m in sorted({max(256, m0 // 2), m0, min(262144, m0 * 2)})}

            def frame_and_summary():
                eng.frame()
                eng.summary(row, counts)
            r["frame_then_summary"] = timed(eng, max(3, a.repeats // 3), 1, frame_and_summary)
            Wp, Wb = pow2_at_least(maxP), pow2_at_least(maxB)
            n1p = Wp if Wp <= m0 else max(m0, Wp // 16)
            mb = min(max(Wb // 4, 256), 262144)
            n1b = Wb if Wb <= mb else max(mb, Wb // 16)
            r["bytes"] = bytes_moved(buf.particle_count, buf.beam_count, maxP, maxB, n1p, n1b)
            r["row"] = row.cpu().tolist()
        out[shape] = r
        eng.destroy()
    print("RESULT " + json.dumps(out), flush=True)


def pass1_from_stats(path, nbytes, calib):
    """the two leaf kernels of a `rocprofv3 --kernel-trace --stats` run of --worker: time per call, bytes/s (config 2 dominates)"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            for key, b in (("k_summary_particles", nbytes["summary_leaf_particles"]), ("k_summary_beams", nbytes["summary_leaf_beams"])):
                if key in r["Name"]:
                    mx = float(r["MaxNs"])
                    rows.append({"kernel": r["Name"], "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3, "max_us": mx / 1e3,
                                 "config2_bytes": b, "config2_gb_per_s_at_max": b / mx,
                                 "of_hbm_calib": (b / mx) / calib if calib else None})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --worker")
    ap.add_argument("--hbm-calib-gbps", type=float, default=None, help="the figure tools/hbm_calib.hip printed on this device")
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

    def fold(label, shape, case, sub=None):
        m = [(r[shape][case][sub] if sub else r[shape][case])["median_ms"] for r in runs[label]]
        return {"medians_ms": m, "ms": statistics.median(m), "spread_ms": max(m) - min(m)}

    res = {"protocol": "wall time of the call(s) + sync(), warm, median of %d; three such medians per case and build, builds alternating, one "
                       "process each; after %d substeps" % (a.repeats, WARM_SUBSTEPS),
           "parent_route": "read_state_device into preallocated tensors + the torch reductions of tools/summary_timing.py parent_route(); "
                           "pending break flags are not reachable on the parent and are left out of its route",
           "shapes": {}}
    for shape in SHAPES:
        first = runs["this"][0][shape]
        t, p = fold("this", shape, "route"), fold("parent", shape, "route")
        s = {"particles": first["particles"], "beams": first["beams"], "capacity": first["capacity"],
             "summary": t, "parent_route": p, "parent_export_only": fold("parent", shape, "export_only"),
             "speedup": p["ms"] / t["ms"], "bar_met": t["ms"] < p["ms"] - p["spread_ms"],
             "sync_only": {"this": fold("this", shape, "sync_only"), "parent": fold("parent", shape, "sync_only")},
             "default_partials": first["default_partials"],
             "partials": {m: fold("this", shape, "partials", m) for m in first["partials"]},
             "frame": {"this": fold("this", shape, "frame"), "parent": fold("parent", shape, "frame")},
             "frame_then_summary": fold("this", shape, "frame_then_summary"),
             "first_call_ms": [r[shape]["first_call_ms"] for r in runs["this"]],
             "table_build_us": [r[shape]["table_build_us"] for r in runs["this"]],
             "bytes": first["bytes"], "row": first["row"]}
        s["default_is_fastest"] = min(s["partials"], key=lambda m: s["partials"][m]["ms"]) == str(first["default_partials"])
        s["summary_gb_per_s_at_most"] = first["bytes"]["summary_total_at_most"] / (t["ms"] * 1e-3) / 1e9
        res["shapes"][shape] = s
    res["bar"] = "summary() < the parent's route - the parent's spread, in both shapes"
    res["bar_met"] = all(s["bar_met"] for s in res["shapes"].values())
    res["hbm_calib_gbps"] = a.hbm_calib_gbps
    if a.stats:
        res["pass1"] = pass1_from_stats(a.stats, res["shapes"]["config2"]["bytes"], a.hbm_calib_gbps)
    import torch
    res = {"device": torch.cuda.get_device_name(0), **res}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
