"""Engine.nearest() against the routes the parent commit offers to the same answer, in the same process.

    python tools/nearest_timing.py [--repeats 7] [--out profiles/nearest_timing.json]

Each scene runs in a process of its own under a time limit.  All times are WALL time of the call plus sync(), warm; a case's figure
is the median of --repeats (at least 7) calls, taken twice with the cases in alternating order (forward, then backward); both
medians are recorded and their mean is the figure.  Shapes:
  config2      bench config 2's scene: a 1000 x 1000 lattice, 1 M particles / 3 M beams, layout v2, bounds 32000, collisions off,
               after 64 substeps
  config3      bench config 3: scenes.config3_buffers(), the blob pile, spatial-hash collisions, settled CONFIG3_SETTLE_FRAMES frames
  nearest()    n = 1, 4096 and 2^20 LOCAL rows drawn in the particles' box with rmax = 4 cells: mask 7 with and without within, mask 1;
               4096 rows with rmax = inf without within; 64 rows with rmax = inf WITH within (the sweep answers them)
  the parent   load_buffers of all four buffers -- the read-back ALONE, the first step of any host route --, and state_tensors()
               plus a chunked torch brute force over the PARTICLES only for the same 4096 rows (no beams: a lower bound of that route)
  beside them  one Engine.raycast of 4096 particle-only rows (mask 5) from the same points
  max_rings    {2, 4, 8, 16, 32} on 4096 mixed rows (mask 7, within, rmax drawn from 0.5 to 6 cells), config2 only
The bar: nearest() of 4096 local rows (mask 7, within on) costs less than the parent's load_buffers alone, on both scenes."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from engine_timing_shapes import config2, config3, timed  # noqa: E402

SHAPES = ("config2", "config3")
WIDTHS = (1, 4096, 1 << 20)
RINGS = (2, 4, 8, 16, 32)
WARM_SUBSTEPS = 64
INF = float("inf")


def worker(a):
    import numpy as np
    import torch
    sb = __import__("__graft_entry__").load_package()
    dev = torch.device("cuda", 0)
    shape = a.worker
    if shape == "config2":
        eng, buf = config2(sb)
        eng.step(WARM_SUBSTEPS)
        bounds = 32000.0
    else:
        eng, buf = config3(sb)
        bounds = float(sb.scenes.config3_buffers()[1])
    eng.sync()
    back = buf.copy()
    eng.load_buffers(back)
    pos = back.particles[back.mapping[:back.particle_count].astype(np.int64), :2]
    box = [float(pos[:, 0].min()), float(pos[:, 1].min()), float(pos[:, 0].max()), float(pos[:, 1].max())]
    G = eng.info("nearest_cells_per_side")
    cell = bounds / G
    r = {"particles": buf.particle_count, "beams": buf.beam_count, "box": box, "cells_per_side": G, "max_rings_default": eng.info("nearest_max_rings")}
    gen = torch.Generator(device=dev).manual_seed(31)
    n_max = max(WIDTHS)
    pts = torch.rand((n_max, 2), generator=gen, device=dev) * torch.tensor([box[2] - box[0], box[3] - box[1]], device=dev) + torch.tensor(box[:2], device=dev)
    out = sb.engine.Nearest(torch.empty(n_max, dtype=torch.float32, device=dev), torch.empty((n_max, 3), dtype=torch.int32, device=dev),
                            torch.empty((n_max, 2), dtype=torch.float32, device=dev), torch.empty((n_max, 2), dtype=torch.int32, device=dev),
                            torch.empty(8, dtype=torch.int64, device=dev))

    def rows(n, rmax, mask):
        return sb.batch.point_rows(pts[None, :n].contiguous(), rmax, mask=mask)[0].contiguous()

    def near(rw, within=True, **kw):
        n = rw.shape[0]
        return lambda: eng.nearest(rw, d=out.d[:n], hit=out.hit[:n], point=out.point[:n], within=out.within[:n] if within else False, counts=out.counts, **kw)

    cases = {}
    for n in WIDTHS:
        local = rows(n, 4.0 * cell, 7)
        cases["local_mask7_within_%d" % n] = near(local)
        cases["local_mask7_%d" % n] = near(local, within=False)
        cases["local_mask1_within_%d" % n] = near(rows(n, 4.0 * cell, 1))
    cases["inf_mask7_4096"] = near(rows(4096, INF, 7), within=False)
    cases["swept_inf_mask7_within_64"] = near(rows(64, INF, 7))
    if shape == "config2":
        mixed = rows(4096, (0.5 + 5.5 * torch.rand(4096, generator=gen, device=dev)) * cell, 7)
        for k in RINGS:
            cases["mixed_4096_max_rings_%d" % k] = near(mixed, max_rings=k)
    # the parent's routes and the ray cast beside them
    cases["parent_load_buffers"] = lambda: eng.load_buffers(back)

    def brute():
        p = eng.state_tensors()["particles"][:, :2]
        for c in range(0, 4096, 128):
            d2 = ((p[None, :, :] - pts[c:c + 128, None, :]) ** 2).sum(-1)
            d2.min(1)
            (d2 <= (4.0 * cell) ** 2).sum(1)
    cases["parent_state_tensors_torch_particles_4096"] = brute
    rays = sb.engine.ray_rows(pts[:4096].contiguous(), torch.tensor([1.0, 0.0], device=dev).expand(4096, 2).contiguous(), INF, mask=5)
    t, hit = torch.empty(4096, dtype=torch.float32, device=dev), torch.empty((4096, 3), dtype=torch.int32, device=dev)
    cases["raycast_mask5_4096"] = lambda: eng.raycast(rays, t=t, hit=hit, counts=out.counts)
    torch.cuda.synchronize()
    names = list(cases)
    for order in (names, names[::-1]):
        for name in order:
            big = name.endswith(str(1 << 20))
            m = timed(eng, a.repeats, 1 if big else 2, cases[name])
            e = r.setdefault(name, {"medians_ms": [], "n": m["n"]})
            e["medians_ms"].append(m["median_ms"])
            if "parent" not in name and "raycast" not in name:
                e["counts"] = out.counts.cpu().tolist()
    for name in names:
        r[name]["ms"] = sum(r[name]["medians_ms"]) / len(r[name]["medians_ms"])
    eng.destroy()
    print("RESULT " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--limit", type=int, default=420, help="seconds per scene's process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("medians of at least 7")
    if a.worker:
        return worker(a)
    res = {"protocol": "wall time of the call + sync(), warm; per case two medians of %d, the cases in forward then backward order; ms = their mean; "
                       "one process per scene under a time limit" % a.repeats,
           "bar": "nearest() of 4096 local rows (mask 7, within on, rmax = 4 cells) < the parent's load_buffers alone, on both scenes", "shapes": {}}
    for shape in SHAPES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", shape, "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=a.limit)
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit("worker %s failed (%d):\n%s" % (shape, p.returncode, p.stderr[-2000:]))   # nothing more is started
        r = json.loads(line[0][7:])
        r["bar_met"] = r["local_mask7_within_4096"]["ms"] < r["parent_load_buffers"]["ms"]
        if shape == "config2":
            r["max_rings_sweep_ms"] = {str(k): r["mixed_4096_max_rings_%d" % k]["ms"] for k in RINGS}
        res["shapes"][shape] = r
        print(shape, {c: round(v["ms"], 4) for c, v in r.items() if isinstance(v, dict) and "ms" in v}, flush=True)
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
