"""What BatchEngine.add_beams costs: 4096 default scenes, 8 welds per scene, timed with HIP events on the batch's
stream, against the only other route to a new beam -- load_scene, a host edit, write_scene, per scene -- timed with the host clock
over 64 scenes of the same batch in the same process and scaled linearly to all scenes (the route is one scene at a time, each with
two waits for the stream, so its cost is per scene); and one frame() before the welds against one after.
Usage: python tools/batch_add_beams_timing.py --out profiles/batch_add_beams_timing.json [--scenes 4096] [--welds 8] [--repeats 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--welds", type=int, default=8)
    ap.add_argument("--host-scenes", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    import batch_add_beams_ref as ref
    ge.build()
    sb = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    n, k = a.scenes, a.welds
    buf = sb.scenes.default_buffers(1, 128, 320)
    be = sb.BatchEngine(n_scenes=n, max_particles=128, max_beams=320)
    be.write_scene(buf)
    rng = np.random.default_rng(3)
    rows = np.zeros((n, k, 8), np.int32)
    for j in range(k):                        # a seeded draw of pairs a != b, different from scene to scene
        rows[:, j, 0] = (rng.integers(0, 119, size=n) + 0) % 119
        rows[:, j, 1] = (rows[:, j, 0] + 1 + rng.integers(0, 117, size=n)) % 119
    rows[:, :, 3:7] = np.asarray(cases_mat(), "f4").view(np.int32)
    drows = torch.from_numpy(rows).cuda()
    stream = torch.cuda.ExternalStream(be.stream())

    def timed(fn):
        """median and minimum of `repeats` runs of fn between two events on the batch's stream, in microseconds"""
        out = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            be.reset()
            be.sync()
            with torch.cuda.stream(stream):
                e0.record()
                fn()
                e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1000.0)
        return float(np.median(out)), float(np.min(out))

    res = torch.empty((n, k), dtype=torch.int32, device="cuda")
    cnt = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    with torch.cuda.stream(stream):
        be.add_beams(drows, length_current=True, result=res, counts=cnt)     # warm
        be.frame()
    be.sync()
    frame_before = timed(lambda: be.frame())
    add = timed(lambda: be.add_beams(drows, length_current=True, result=res, counts=cnt))

    def frame_after():
        be.add_beams(drows, length_current=True, result=res, counts=cnt)
    out_after = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        be.reset()
        with torch.cuda.stream(stream):
            frame_after()
            e0.record()
            be.frame()
            e1.record()
        e1.synchronize()
        out_after.append(e0.elapsed_time(e1) * 1000.0)
    added = int(cnt[:, 0].sum().item())
    # the host route, one scene at a time (it also replaces the scene's reset state)
    be.reset()
    be.sync()
    m = min(a.host_scenes, n)
    t0 = time.perf_counter()
    for i in range(m):
        got = be.load_scene(i, buf.copy())
        edited, _, _ = ref.add_ref(got, rows[i], ref.LENGTH_CURRENT, None)
        be.write_scene(edited, i, 1)
    be.sync()
    host_us = (time.perf_counter() - t0) * 1e6
    t0 = time.perf_counter()
    for i in range(m):
        ref.add_ref(buf, rows[i], ref.LENGTH_CURRENT, None)
    edit_us = (time.perf_counter() - t0) * 1e6
    result = dict(
        what="BatchEngine.add_beams against load_scene + host edit + write_scene, and a frame before / after the welds",
        device=torch.cuda.get_device_name(0), scenes=n, welds_per_scene=k, beams_added=added, repeats=a.repeats,
        add_beams_us=dict(median=add[0], min=add[1]), add_beams_kernel_vgprs=be.info("add_beams_kernel_vgprs"),
        host_route=dict(scenes_timed=m, total_us=host_us, per_scene_us=host_us / m, of_which_numpy_edit_us_per_scene=edit_us / m,
                        scaled_to_all_scenes_us=host_us / m * n,
                        scaling="linear in the scenes: the route handles one scene per call and waits for the stream twice per scene"),
        ratio_host_route_over_add_beams=host_us / m * n / add[0],
        frame_us=dict(before_welds=dict(median=frame_before[0], min=frame_before[1]),
                      after_welds=dict(median=float(np.median(out_after)), min=float(np.min(out_after)))))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    be.destroy()


def cases_mat():
    return (1.0, 50.0, 1.0, 2.5)


if __name__ == "__main__":
    main()
