"""sb_render_device time from device events (warm, median of N renders) and the first render's draw-table build.

    python tools/render_timing.py [--repeats 25] [--out profiles/render_timing.json]

Scenes: BASELINE config 2 (a 1000 x 1000 lattice, 1 M particles / 3 M beams, bounds 32000, collisions off) after 20 substeps at
1024^2 and 4096^2; the default scene (119 particles / 299 beams, bounds 1000) after 2 frames at 1000^2.  Each render is bracketed
by two sb_mark events on the engine's stream into a uint8 torch tensor; nothing else runs between the marks."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(eng, dst, res, repeats):
    eng.render_device(dst, res)   # warm: tables, key image
    eng.sync()
    ms = []
    for _ in range(repeats):
        eng.mark(0)
        eng.render_device(dst, res)
        eng.mark(1)
        ms.append(eng.mark_elapsed(0, 1))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "renders": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    sb = ge.load_package()
    rows = []

    buf = sb.scenes.lattice_buffers(1000, 1000, d=30.0, origin=(1000.0, 1000.0), jitter=1.0, layout=2)
    eng = sb.Engine(bounds_size=32000.0, layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=0)
    eng.write_buffers(buf)
    eng.step(20)
    eng.sync()
    dst = torch.empty(4096 * 4096 * 3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    t = time.perf_counter()
    eng.render(1024)
    first_ms = (time.perf_counter() - t) * 1e3
    build = eng.info("render_table_build_us") / 1e3
    frame_ms = eng.step_timed(64)
    for res in (1024, 4096):
        r = timed(eng, dst, res, a.repeats)
        r.update(scene="config 2: 1000x1000 lattice, P=%d B=%d, bounds 32000, after 20 substeps" % (buf.particle_count, buf.beam_count),
                 resolution=res)
        rows.append(r)
    rows.append({"scene": "config 2", "first_render_wall_ms": first_ms, "table_build_host_ms": build,
                 "frame_64_substeps_device_ms": frame_ms})
    eng.destroy()

    d = sb.scenes.default_buffers(1, 256, 512)
    eng = sb.Engine(layout=1, max_particles=256, max_beams=512)
    eng.write_buffers(d)
    eng.frame()
    eng.frame()
    eng.sync()
    r = timed(eng, dst, 1000, a.repeats)
    r.update(scene="default scene: P=%d B=%d, bounds 1000, after 2 frames" % (d.particle_count, d.beam_count), resolution=1000)
    rows.append(r)
    eng.destroy()

    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
