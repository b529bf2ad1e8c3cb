"""Engine.checkpoint / restore / write_beams_device against the only routes the parent commit has to the same ends (DESIGN.md 5.9.1,
5.9.2).

    python tools/checkpoint_timing.py [--repeats 50] [--out profiles/checkpoint_timing.json] [--bench bench_runs.json]

Scene: BASELINE config 2 (a 1000 x 1000 lattice, 1 M particles / 3 M beams, layout v2, bounds 32000) after 20 substeps, with
collisions off (the blocked layout) and with the default collision mode (tiled layout + hybrid).  The protocol of
tools/state_io_timing.py: one process, the new call and its baseline alternating after a warm-up, each timed on the host clock from
an idle stream to the end of a synchronise, median of --repeats.
  (a) checkpoint, and restore, each against sb_load_buffers + a plan-keeping sb_write_buffers of those bytes (going back through the
      host).  Every upload drops the checkpoint, so each round takes one untimed checkpoint (the allocating one, reported apart as
      first_checkpoint) before the timed one.
  (b) write_beams_device (both fields) against a plan-keeping sb_write_buffers of the edited records.
  (c) a frame right after a restore against a frame in steady state (the forced hash build, the hybrid's fresh look).
  (d) the enqueue cost of a restore (host clock around the call alone, no synchronise) and the number of copies it issues.
--bench merges a JSON file of interleaved bench.py runs (parent / branch) into the result."""
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


def measure(sb, torch, buf, mode, name, a):
    maxP, maxB = buf.max_particles, buf.max_beams
    eng = sb.Engine(bounds_size=32000.0, layout=2, max_particles=maxP, max_beams=maxB, collision_mode=mode)
    eng.write_buffers(buf)
    eng.step(20)
    eng.sync()
    host = buf.copy()
    res = {"collision_mode": name, "path": eng.kernel_name()}

    def back_through_the_host():
        eng.load_buffers(host)
        eng.write_buffers(host)

    kept0 = eng.info("uploads_kept")
    first, ck, rs, rs_enq, base = [], [], [], [], []
    for i in range(a.warmup + a.repeats):
        b = host_ms(eng, back_through_the_host)
        f = host_ms(eng, eng.checkpoint)        # the first one after an upload allocates
        c = host_ms(eng, eng.checkpoint)
        eng.step(3)
        r = host_ms(eng, eng.restore)
        eng.step(3)
        q = enqueue_ms(eng, eng.restore)
        if i >= a.warmup:
            base.append(b), first.append(f), ck.append(c), rs.append(r), rs_enq.append(q)
    assert eng.info("uploads_kept") - kept0 == a.warmup + a.repeats, "every upload must keep the plan"
    res["checkpoint_bytes"] = eng.info("checkpoint_bytes")
    res["load_plus_write_buffers_host"] = summary(base)
    res["first_checkpoint_host"] = summary(first)
    res["checkpoint_host"] = summary(ck)
    res["restore_host"] = summary(rs)
    res["restore_enqueue_only_host"] = summary(rs_enq)
    res["checkpoint_speedup"] = res["load_plus_write_buffers_host"]["median_ms"] / res["checkpoint_host"]["median_ms"]
    res["restore_speedup"] = res["load_plus_write_buffers_host"]["median_ms"] / res["restore_host"]["median_ms"]
    # copies both directions move checkpoint_bytes once in and once out of HBM
    res["restore_achieved_TBps"] = 2.0 * res["checkpoint_bytes"] / (res["restore_host"]["median_ms"] * 1e-3) / 1e12

    # (b) beam import against a plan-keeping upload of the edited records
    t = eng.state_tensors()
    rows = t["beams"] * 1.0
    rows[:, 0] *= 0.999
    state = eng.load_buffers(buf.copy())
    state.beams["target_length"] *= 0.999
    torch.cuda.synchronize()
    imp = lambda: eng.write_beams_device(rows, True, True)      # noqa: E731
    res["first_write_beams_device_host_ms"] = host_ms(eng, imp)  # builds its tables
    up, im = [], []
    for i in range(a.warmup + a.repeats):
        u = host_ms(eng, lambda: eng.write_buffers(state))
        host_ms(eng, imp)                                        # (the first one after an upload builds the tables)
        m = host_ms(eng, imp)
        if i >= a.warmup:
            up.append(u), im.append(m)
    res["write_buffers_plan_kept_host"] = summary(up)
    res["write_beams_device_host"] = summary(im)
    res["beam_import_table_build_us"] = eng.info("beam_import_table_build_us")
    res["write_beams_speedup"] = res["write_buffers_plan_kept_host"]["median_ms"] / res["write_beams_device_host"]["median_ms"]

    # (c) a frame right after a restore against a frame in steady state
    eng.write_buffers(buf)
    for _ in range(3):
        eng.frame()
    eng.checkpoint()
    steady, after = [], []
    for _ in range(10):
        steady.append(host_ms(eng, eng.frame))
    for _ in range(10):
        eng.restore()
        after.append(host_ms(eng, eng.frame))
    res["frame_steady_host"] = summary(steady)
    res["frame_after_restore_host"] = summary(after)
    for k in ("checkpoint", "restore", "write_beams"):
        res["bar_10x_" + k] = res[k + "_speedup"] >= 10.0
    eng.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench", default=None, help="JSON of interleaved bench.py runs to merge (parent / branch)")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    sb = ge.load_package()
    buf = sb.scenes.lattice_buffers(1000, 1000, d=30.0, origin=(1000.0, 1000.0), jitter=1.0, layout=2)
    res = {"scene": "config 2: 1000x1000 lattice, P=%d B=%d, layout v2, bounds 32000, after 20 substeps" % (buf.particle_count, buf.beam_count),
           "protocol": "host clock, idle stream to the end of a synchronise, median of %d, new call and baseline alternating in one process" % a.repeats,
           "runs": [measure(sb, torch, buf, 0, "off", a), measure(sb, torch, buf, 2, "grid (default)", a)]}
    if a.bench:
        with open(a.bench) as f:
            res["bench_headline"] = json.load(f)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), **res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
