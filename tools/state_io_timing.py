"""sb_read_state_device / sb_write_particles_device against the host round trips they replace.

    python tools/state_io_timing.py [--repeats 50] [--out profiles/state_io_timing.json] [--stats kernel_stats.csv]

Scene: BASELINE config 2 (a 1000 x 1000 lattice, 1 M particles / 3 M beams, layout v2, bounds 32000, collisions off) after 20
substeps.  Everything runs in one process, the new call and its baseline alternating, after a warm-up:
  (a) read_state_device of all three outputs into torch tensors, against sb_load_buffers of the same state (metadata, mapping,
      particles, beams into host buffers);
  (b) write_particles_device of the exported particle records, against a plan-keeping sb_write_buffers of the same particle bytes.
Each call is timed on the host clock from an idle stream to the end of a synchronise (median of --repeats); the new calls also
by two sb_mark events around them.  The first export after an upload builds its tables and is reported apart.
--stats merges the kernel statistics of a separate `rocprofv3 --kernel-trace --stats` run of this tool (kernel_stats.csv) and
gives each kernel's achieved bytes/s against the bytes computed here."""
import argparse
import csv
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


def device_ms(eng, fn):
    eng.mark(0)
    fn()
    eng.mark(1)
    return eng.mark_elapsed(0, 1)


def kernel_bytes(P, B):
    """HBM bytes each kernel has to move (every array element read or written once)"""
    return {
        # pos, vel, acc in (8 B each) + the data index (4 B) + the 24-byte record out
        "k_state_export_particles": P * (24 + 4 + 24),
        # per caller slot: {engine slot, data index} (8 B) + its copy (4 B) + 4 state floats in + 16 B out + the live byte
        "k_state_export_beams": B * (8 + 4 + 16 + 16 + 1),
        # the data index (4 B) + the 24-byte record in + pos, vel, acc out
        "k_state_import_particles": P * (4 + 24 + 24),
    }


def merge_stats(path, nbytes):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            key = next((k for k in sorted(nbytes, key=len, reverse=True) if name.startswith("void " + k + "(") or name.startswith(k + "(")), None)
            if key is None:
                continue
            avg_ns = float(r["AverageNs"])
            rows.append({"kernel": key, "calls": int(r["Calls"]), "average_us": avg_ns / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                         "bytes": nbytes[key], "achieved_TBps": nbytes[key] / avg_ns / 1e3})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    sb = ge.load_package()
    buf = sb.scenes.lattice_buffers(1000, 1000, d=30.0, origin=(1000.0, 1000.0), jitter=1.0, layout=2)
    P, B, maxP, maxB = buf.particle_count, buf.beam_count, buf.max_particles, buf.max_beams
    eng = sb.Engine(bounds_size=32000.0, layout=2, max_particles=maxP, max_beams=maxB, collision_mode=0)
    eng.write_buffers(buf)
    eng.step(20)
    eng.sync()
    dev = torch.device("cuda", 0)
    tp = torch.empty((maxP, 6), dtype=torch.float32, device=dev)
    tb = torch.empty((maxB, 4), dtype=torch.float32, device=dev)
    ta = torch.empty(maxB, dtype=torch.uint8, device=dev)
    host = buf.copy()
    torch.cuda.synchronize()
    export = lambda: eng.read_state_device(tp, tb, ta)          # noqa: E731
    first_ms = host_ms(eng, export)                              # builds the beam tables
    res = {"scene": "config 2: 1000x1000 lattice, P=%d B=%d, layout v2, bounds 32000, collisions off, after 20 substeps" % (P, B),
           "first_export_wall_ms": first_ms}

    # (a) export against sb_load_buffers
    load = lambda: eng.load_buffers(host)                       # noqa: E731
    for _ in range(a.warmup):
        host_ms(eng, export)
        host_ms(eng, load)
    ex_h, ex_d, ld_h = [], [], []
    for _ in range(a.repeats):
        ex_h.append(host_ms(eng, export))
        eng.sync()
        ex_d.append(device_ms(eng, export))
        ld_h.append(host_ms(eng, load))
    res["read_state_device_host"] = summary(ex_h)
    res["read_state_device_events"] = summary(ex_d)
    res["load_buffers_host"] = summary(ld_h)
    res["export_speedup"] = res["load_buffers_host"]["median_ms"] / res["read_state_device_host"]["median_ms"]

    # (b) import against a plan-keeping sb_write_buffers of the same particle bytes
    eng.read_state_device(tp)
    state = eng.load_buffers(buf.copy())
    torch.cuda.synchronize()
    kept0 = eng.info("uploads_kept")
    imp = lambda: eng.write_particles_device(tp)                # noqa: E731
    upload = lambda: eng.write_buffers(state)                   # noqa: E731
    for _ in range(a.warmup):
        host_ms(eng, imp)
        host_ms(eng, upload)
    im_h, im_d, up_h = [], [], []
    for _ in range(a.repeats):
        im_h.append(host_ms(eng, imp))
        eng.sync()
        im_d.append(device_ms(eng, imp))
        up_h.append(host_ms(eng, upload))
    kept = eng.info("uploads_kept") - kept0
    assert kept == a.warmup + a.repeats, "every upload must keep the plan (%d of %d did)" % (kept, a.warmup + a.repeats)
    res["write_particles_device_host"] = summary(im_h)
    res["write_particles_device_events"] = summary(im_d)
    res["write_buffers_plan_kept_host"] = summary(up_h)
    res["import_speedup"] = res["write_buffers_plan_kept_host"]["median_ms"] / res["write_particles_device_host"]["median_ms"]
    res["bar_10x_export"] = res["export_speedup"] >= 10.0
    res["bar_10x_import"] = res["import_speedup"] >= 10.0
    eng.destroy()

    nbytes = kernel_bytes(P, B)
    res["kernel_bytes"] = nbytes
    if a.stats:
        res["kernels"] = merge_stats(a.stats, nbytes)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), **res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
