"""BatchEngine against the loop a user writes without it.

    python tools/batch_timing.py [--repeats 25] [--out profiles/batch_timing.json] [--sizes 256,4096,32768]

Everything in one process, warm, median of --repeats, one frame of 64 substeps + the delete pass:
  baseline  ONE sb.Engine on the default scene (119 particles / 299 beams), wall clock per frame() + sync(), for collision_mode
            ALLPAIRS and for the default GRID; the better of the two is t1.  N scenes done that way cost N * t1 (the engines share
            one GPU and each frame is a chain of dependent launches).
  batch     BatchEngine with N scenes of the default scene, collisions on: HIP events on the batch's stream around frame(); tN / N
            per scene-frame.  Also N = 4096 of a 32 x 32 lattice (1024 particles: the O(P^2) walk at the capacity limit) with
            collisions on and off.
The bar: at N = 4096 the batch's time per scene-frame is at most t1 / 32."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def engine_frame_ms(sb, buf, mode, repeats, warmup):
    eng = sb.Engine(layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=mode)
    eng.write_buffers(buf)
    for _ in range(warmup):
        eng.frame()
    eng.sync()
    ms = []
    for _ in range(repeats):
        t = time.perf_counter()
        eng.frame()
        eng.sync()
        ms.append((time.perf_counter() - t) * 1e3)
    eng.destroy()
    return summary(ms)


def batch_frame_ms(sb, torch, buf, n, mode, repeats, warmup):
    be = sb.BatchEngine(n_scenes=n, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=mode)
    be.write_scene(buf)
    stream = torch.cuda.ExternalStream(be.stream(), device=torch.device("cuda", 0))
    for _ in range(warmup):
        be.frame()
    be.sync()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        be.frame()
        e1.record(stream)
        be.sync()
        ms.append(e0.elapsed_time(e1))
    r = summary(ms)
    r.update(n_scenes=n, per_scene_frame_us=r["median_ms"] * 1e3 / n,
             **{k: be.info(k) for k in ("threads_per_scene", "lds_bytes_per_scene", "materials_in_lds", "scenes_per_cu",
                                        "frame_kernel_vgprs", "frame_kernel_scratch_bytes")})
    be.destroy()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="256,4096,32768")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    sb = ge.load_package()
    small = sb.scenes.default_buffers(1, 128, 320)
    res = {"scene": "the reference's default scene, 119 particles / 299 beams, v1, capacity 128 / 320, subticks 64, one frame",
           "engine_allpairs": engine_frame_ms(sb, small, 1, a.repeats, a.warmup),
           "engine_grid": engine_frame_ms(sb, small, 2, a.repeats, a.warmup)}
    t1 = min(res["engine_allpairs"]["median_ms"], res["engine_grid"]["median_ms"])
    res["t1_ms"] = t1
    res["batch"] = []
    for n in [int(x) for x in a.sizes.split(",") if x]:
        r = batch_frame_ms(sb, torch, small, n, 2, a.repeats, a.warmup)
        r["speedup_over_n_engines"] = t1 * 1e3 / r["per_scene_frame_us"]
        res["batch"].append(r)
        print(json.dumps(r), flush=True)
    at4096 = next((r for r in res["batch"] if r["n_scenes"] == 4096), None)
    if at4096:
        res["bar"] = "per scene-frame at N = 4096 <= t1 / 32"
        res["bar_met"] = at4096["per_scene_frame_us"] <= t1 * 1e3 / 32.0
    lat = sb.scenes.lattice_buffers(32, 32, d=25.0, origin=(100.0, 100.0), strain_limit=0.5, jitter=2.0, layout=2)
    big = sb.Buffers(2, 1024, 4096)
    big.set_scene(lat.particles[:1024], lat.beams[:lat.beam_count].copy())
    res["lattice_32x32_collisions_on"] = batch_frame_ms(sb, torch, big, 4096, 2, max(3, a.repeats // 5), 1)
    res["lattice_32x32_collisions_off"] = batch_frame_ms(sb, torch, big, 4096, 0, max(3, a.repeats // 5), 1)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), **res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
