"""BatchEngine.render against one Engine.render_device per scene.

    python tools/batch_render_timing.py [--repeats 25] [--out profiles/batch_render_timing.json] [--sizes 256,4096,32768]

Everything in one process, warm, median of --repeats, the default scene (119 particles / 299 beams) after 3 frames:
  baseline  t1(res): device time of ONE Engine.render_device at that resolution, between two marks on the engine's stream (as
            tools/render_timing.py measures it)
  batch     HIP events on the batch's stream around one render of N scenes at 64^2 / 84^2 / 128^2 / 256^2 into a preallocated
            device buffer; time per picture, written bytes per second, and the ratio to the sb_batch_frame of the same batch
  budget    at N = 4096: the same with the LDS budget of a workgroup (SB_BATCH_RENDER_LDS_BYTES) set to 40 / 80 / 160 KiB
The bar: at N = 4096 the batch's device time per picture is at most t1(res) / 32, for res 64 and 128."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RESOLUTIONS = (64, 84, 128, 256)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def engine_render_ms(eng, dst, res, repeats):
    eng.render_device(dst, res)
    eng.sync()
    ms = []
    for _ in range(repeats):
        eng.mark(0)
        eng.render_device(dst, res)
        eng.mark(1)
        ms.append(eng.mark_elapsed(0, 1))
    return summary(ms)


def timed(torch, be, stream, call, repeats):
    call()
    be.sync()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        be.sync()
        ms.append(e0.elapsed_time(e1))
    return summary(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--sizes", default="256,4096,32768")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    sb = ge.load_package()
    buf = sb.scenes.default_buffers(1, 128, 320)
    sizes = [int(x) for x in a.sizes.split(",") if x]
    dst = torch.empty(max(sizes) * max(RESOLUTIONS) ** 2 * 3, dtype=torch.uint8, device="cuda:0")
    res = {"scene": "the reference's default scene, 119 particles / 299 beams, v1, capacity 128 / 320, after 3 frames"}

    eng = sb.Engine(layout=1, max_particles=128, max_beams=320)
    eng.write_buffers(buf)
    for _ in range(3):
        eng.frame()
    eng.sync()
    res["t1_ms"] = {str(r): engine_render_ms(eng, dst, r, a.repeats) for r in RESOLUTIONS}
    eng.destroy()
    print(json.dumps(res["t1_ms"]), flush=True)

    res["batch"] = []
    for n in sizes:
        be = sb.BatchEngine(n_scenes=n, layout=1, max_particles=128, max_beams=320)
        be.write_scene(buf)
        be.frame(3)
        be.sync()
        stream = torch.cuda.ExternalStream(be.stream(), device=torch.device("cuda", 0))
        frame = timed(torch, be, stream, lambda: be.frame(1), max(3, a.repeats // 5))
        be.reset()
        be.frame(3)
        be.sync()
        budgets = [None] + ([40, 80, 160] if n == 4096 else [])
        for kib in budgets:
            if kib is None:
                os.environ.pop("SB_BATCH_RENDER_LDS_BYTES", None)
            else:
                os.environ["SB_BATCH_RENDER_LDS_BYTES"] = str(kib * 1024)
            for r in RESOLUTIONS:
                row = timed(torch, be, stream, lambda: be.render(r, out=dst.data_ptr()), a.repeats)
                t1 = res["t1_ms"][str(r)]["median_ms"]
                row.update(n_scenes=n, resolution=r, lds_budget_kib=kib, per_picture_us=row["median_ms"] * 1e3 / n,
                           t1_over_per_picture=t1 * n / row["median_ms"], written_gb_per_s=n * r * r * 3 / row["median_ms"] / 1e6,
                           render_over_frame=row["median_ms"] / frame["median_ms"], frame_ms=frame["median_ms"],
                           **{k: be.info(k) for k in ("render_bands", "render_lds_bytes", "render_kernel_vgprs",
                                                      "render_kernel_scratch_bytes")})
                res["batch"].append(row)
                print(json.dumps(row), flush=True)
        os.environ.pop("SB_BATCH_RENDER_LDS_BYTES", None)
        be.destroy()
    bar = [r for r in res["batch"] if r["n_scenes"] == 4096 and r["lds_budget_kib"] is None and r["resolution"] in (64, 128)]
    if bar:
        res["bar"] = "device time per picture at N = 4096 <= t1(res) / 32, for res 64 and 128"
        res["bar_met"] = all(r["t1_over_per_picture"] >= 32.0 for r in bar)
    print(json.dumps({k: res[k] for k in ("bar", "bar_met") if k in res}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), **res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
