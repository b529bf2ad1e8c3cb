"""Engine.cut + delete_pass and BatchEngine.cut + delete_pass against the only route the parent commit has to the same removal: read
the scene back, remove the beams on the host, upload again.

    python tools/cut_timing.py [--repeats 20] [--warmup 3] [--out profiles/cut_timing.json] [--skip-batch]

Engine: BASELINE config 2 (a 1000 x 1000 lattice, 1 M particles / 3 M beams, layout v2, bounds 32000, collisions off) after 20
substeps.  Two removals: "stroke", one knife across the whole lattice; "discs", 64 eraser discs sized so that about 1 % of the beams
lie under them.  The protocol of tools/checkpoint_timing.py: one process, the new route and its baseline alternating after a
warm-up, each timed on the host clock from an idle stream to the end of a synchronise, median of --repeats.  Every round starts
from the same state: an untimed upload of the uncut scene (which keeps the plan) and 20 substeps.
  new       sb_cut_device (shapes already in device memory, counts asked for) + sb_delete_pass
  baseline  sb_load_buffers + the host pass that drops the hit beams' slots (numpy, the hit set known in advance: the predicate is
            not timed on the host) + the plan-keeping sb_write_buffers of the edited scene, as tests/test_gpu_reupload.py does it
  also      the first cut after an upload (it builds its tables and waits once), a dry run, and the enqueue cost alone
Batch: 4096 default scenes (119 particles / 299 beams each), every scene cut by its own stroke; sb_batch_cut_device +
sb_batch_delete_pass against load_scene + the same host pass + write_scene per scene, timed over --batch-baseline-scenes scenes
and scaled to the batch (the route is one scene at a time: its cost is linear in the scenes)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def host_ms(eng, fn):
    eng.sync()
    t = time.perf_counter()
    fn()
    eng.sync()
    return (time.perf_counter() - t) * 1e3


def enqueue_ms(eng, fn):
    eng.sync()
    t = time.perf_counter()
    fn()
    dt = (time.perf_counter() - t) * 1e3
    eng.sync()
    return dt


def without(buf, hit_by_data_index):
    """`buf` (a read-back) without the beam slots whose record is hit: slots and records renumbered in order (what
    BufferMapper.writeState leaves of a scene after removeBeam calls; tests/test_gpu_reupload.py `without`)"""
    out = buf.copy()
    maxP, nb = buf.max_particles, buf.beam_count
    d = buf.mapping[maxP:maxP + nb].astype(np.int64)
    recs = buf.beams[d][hit_by_data_index[d] == 0]
    n = len(recs)
    out.beams[:n] = recs
    out.mapping[maxP:maxP + n] = np.arange(n, dtype=out.mapping.dtype)
    out.beam_count = n
    return out


def engine_shapes(sb, buf):
    p = buf.particles[:buf.particle_count, :2]
    x0, y0, x1, y1 = float(p[:, 0].min()), float(p[:, 1].min()), float(p[:, 0].max()), float(p[:, 1].max())
    w, h = x1 - x0, y1 - y0
    # 64 discs on an 8 x 8 grid covering 1 % of the lattice's area together: pi r^2 * 64 = 0.01 w h
    r = (0.01 * w * h / (64.0 * np.pi)) ** 0.5
    discs = [(x0 + w * (i + 0.5) / 8, y0 + h * (j + 0.5) / 8, r) for i in range(8) for j in range(8)]
    return {"stroke": sb.cut_shapes(segments=[(x0 - 10, y0 + 0.37 * h, x1 + 10, y0 + 0.61 * h)]), "discs": sb.cut_shapes(discs=discs)}


def measure_engine(sb, torch, a):
    buf = sb.scenes.lattice_buffers(1000, 1000, d=30.0, origin=(1000.0, 1000.0), jitter=1.0, layout=2)
    eng = sb.Engine(bounds_size=32000.0, layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=0)
    eng.write_buffers(buf)
    res = {"scene": "config 2: 1000x1000 lattice, P=%d B=%d, layout v2, bounds 32000, collisions off, after 20 substeps" % (buf.particle_count, buf.beam_count),
           "path": eng.kernel_name(), "cases": {}}
    host = buf.copy()

    def fresh():
        eng.write_buffers(buf)
        eng.step(20)
        eng.sync()

    for name, rows in engine_shapes(sb, buf).items():
        shapes = torch.from_numpy(rows.view(np.int32)).cuda()
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        hit = torch.zeros(buf.max_beams, dtype=torch.uint8, device="cuda")
        fresh()
        first = host_ms(eng, lambda: eng.cut(shapes, dry_run=True, hit=hit, counts=counts))   # builds the tables
        hit_host = hit.cpu().numpy()
        c = counts.cpu().numpy().tolist()
        new, base, dry, enq = [], [], [], []

        def cut_and_delete():
            eng.cut(shapes, counts=counts)
            eng.delete_pass()

        def through_the_host():
            eng.load_buffers(host)
            eng.write_buffers(without(host, hit_host))

        kept0 = eng.info("uploads_kept")
        for i in range(a.warmup + a.repeats):
            fresh()
            eng.cut(shapes, dry_run=True, counts=counts)      # (untimed: the first call after an upload builds the tables)
            d = host_ms(eng, lambda: eng.cut(shapes, dry_run=True, counts=counts))
            q = enqueue_ms(eng, lambda: eng.cut(shapes, dry_run=True, counts=counts))
            n = host_ms(eng, cut_and_delete)
            after_new = eng.counts()[1]
            fresh()
            b = host_ms(eng, through_the_host)
            assert eng.counts()[1] == after_new == buf.beam_count - c[1], "both routes must remove the same beams"
            if i >= a.warmup:
                new.append(n), base.append(b), dry.append(d), enq.append(q)
        kept = eng.info("uploads_kept") - kept0   # (3 uploads a round; the baseline's must keep the plan to be the parent's best route)
        r = {"counts": dict(zip(sb.CUT_COUNT_FIELDS, c)), "fraction_of_beams_cut": c[1] / buf.beam_count,
             "uploads_that_kept_the_plan": [int(kept), 3 * (a.warmup + a.repeats)], "first_cut_after_upload_host_ms": first, "cut_table_build_us": eng.info("cut_table_build_us"),
             "cut_plus_delete_pass_host": summary(new), "load_edit_write_buffers_host": summary(base), "dry_run_host": summary(dry),
             "dry_run_enqueue_only_host": summary(enq)}
        r["speedup"] = r["load_edit_write_buffers_host"]["median_ms"] / r["cut_plus_delete_pass_host"]["median_ms"]
        res["cases"][name] = r
    res["cut_kernel_vgprs"] = eng.info("cut_kernel_vgprs")
    eng.destroy()
    return res


def measure_batch(sb, torch, a):
    n = 4096
    buf = sb.Buffers(2, 128, 320)
    dp, db = sb.scenes.default_scene(2)
    buf.set_scene(dp, db)
    be = sb.BatchEngine(n_scenes=n, layout=2, max_particles=128, max_beams=320)
    rng = np.random.default_rng(1)
    segs = np.stack([np.full(n, -10.0), rng.uniform(0, 1000, n), np.full(n, 1010.0), rng.uniform(0, 1000, n)], axis=1)
    rows = np.stack([sb.cut_shapes(segments=[s]) for s in segs])   # [n, 1, 8]: a different stroke per scene
    shapes = torch.from_numpy(rows.view(np.int32)).cuda()
    counts = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    hit = torch.zeros((n, 320), dtype=torch.uint8, device="cuda")
    m = min(a.batch_baseline_scenes, n)
    host = [buf.copy() for _ in range(m)]

    def fresh():
        be.write_scene(buf)
        be.step(20)
        be.sync()

    fresh()
    be.cut(shapes, dry_run=True, hit=hit, counts=counts)
    be.sync()
    hit_host = hit.cpu().numpy()

    def cut_and_delete():
        be.cut(shapes, counts=counts)
        be.delete_pass()

    def through_the_host():
        for i in range(m):
            be.load_scene(i, host[i])
            be.write_scene(without(host[i], hit_host[i]), i, 1)

    new, base = [], []
    for i in range(a.warmup + a.repeats):
        fresh()
        t = host_ms(be, cut_and_delete)
        fresh()
        b = host_ms(be, through_the_host)
        if i >= a.warmup:
            new.append(t), base.append(b * n / m)
    res = {"scene": "%d default scenes (119 particles / 299 beams), a different stroke each, after 20 substeps" % n,
           "beams_cut_per_scene_mean": float(hit_host.sum() / n), "baseline_timed_over_scenes": m,
           "batch_cut_plus_delete_pass_host": summary(new), "load_scene_edit_write_scene_host_scaled_to_batch": summary(base),
           "cut_kernel_vgprs": be.info("cut_kernel_vgprs")}
    res["speedup"] = res["load_scene_edit_write_scene_host_scaled_to_batch"]["median_ms"] / res["batch_cut_plus_delete_pass_host"]["median_ms"]
    be.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch-baseline-scenes", type=int, default=256)
    ap.add_argument("--skip-batch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    sb = ge.load_package()
    res = {"protocol": "host clock, idle stream to the end of a synchronise, median of %d, new route and baseline alternating in one process, "
                       "every round from a fresh plan-keeping upload + 20 substeps" % a.repeats,
           "engine": measure_engine(sb, torch, a)}
    if not a.skip_batch:
        res["batch"] = measure_batch(sb, torch, a)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), **res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
