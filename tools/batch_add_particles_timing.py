"""What BatchEngine.add_particles costs: 4096 default scenes, 8 spawned particles per scene, timed with HIP events
on the batch's stream (medians of 20), against the only other route to a new particle -- load_scene, a numpy edit, write_scene, per
scene -- timed with the host clock over 64 scenes of the same batch and scaled linearly to all scenes (the route is one scene at a
time, each with two waits for the stream); and reset() and frame() of scenes that never had a particle added, which the change to
k_batch_reset sits on, against the same two calls of another checkout (the parent commit) on the same machine.
Usage:
  python tools/batch_add_particles_timing.py --reset-frame-only --package-root PARENT_CHECKOUT --out parent.json   (the parent: built already)
  python tools/batch_add_particles_timing.py --parent parent.json --out profiles/batch_add_particles_timing.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--host-scenes", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose package and library are measured")
    ap.add_argument("--reset-frame-only", action="store_true", help="measure reset() and frame() only (a checkout without add_particles)")
    ap.add_argument("--parent", help="the JSON a --reset-frame-only run of the parent commit wrote: merged into the output")
    a = ap.parse_args()
    root = os.path.abspath(a.package_root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import __graft_entry__ as ge
    if root == ROOT:
        ge.build()
    sb = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    n, k = a.scenes, a.rows
    buf = sb.scenes.default_buffers(1, 128, 320)
    be = sb.BatchEngine(n_scenes=n, max_particles=128, max_beams=320)
    be.write_scene(buf)
    stream = torch.cuda.ExternalStream(be.stream())

    def timed(fn, before=lambda: None):
        """median and minimum of `repeats` runs of fn between two events on the batch's stream, in microseconds; `before` runs
        ahead of the first event"""
        out = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                before()
                be.sync()
                e0.record()
                fn()
                e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1000.0)
        return dict(median=float(np.median(out)), min=float(np.min(out)), max=float(np.max(out)))

    with torch.cuda.stream(stream):
        be.frame()
        be.reset()
    be.sync()
    # scenes that never had a particle added: reset after a frame, and a frame from the reset state
    result = dict(device=torch.cuda.get_device_name(0), scenes=n, repeats=a.repeats,
                  reset_us=timed(lambda: be.reset(), before=lambda: be.frame()),
                  frame_us=timed(lambda: be.frame(), before=lambda: be.reset()))
    if not a.reset_frame_only:
        import batch_add_particles_ref as ref
        rng = np.random.default_rng(5)
        rows = np.zeros((n, k, 8), np.int32)
        pos = np.empty((n, k, 2), "f4")                   # a seeded draw in the empty middle of the box, different from scene to scene
        pos[:, :, 0], pos[:, :, 1] = rng.uniform(300.0, 650.0, (n, k)), rng.uniform(250.0, 380.0, (n, k))
        rows[:, :, 1:3] = pos.view(np.int32)
        drows = torch.from_numpy(rows).cuda()
        res = torch.empty((n, k), dtype=torch.int32, device="cuda")
        cnt = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        with torch.cuda.stream(stream):
            be.add_particles(drows, result=res, counts=cnt)      # warm
            be.reset()
        be.sync()
        add = timed(lambda: be.add_particles(drows, result=res, counts=cnt), before=lambda: be.reset())
        skip = timed(lambda: be.add_particles(drows, skip_touching=True, result=res, counts=cnt), before=lambda: be.reset())
        be.reset()
        be.add_particles(drows, result=res, counts=cnt)
        added = int(cnt[:, 0].sum().item())
        frame_after = timed(lambda: be.frame(), before=lambda: (be.reset(), be.add_particles(drows, result=res, counts=cnt)))
        reset_after = timed(lambda: be.reset(), before=lambda: be.add_particles(drows, result=res, counts=cnt))
        # the host route, one scene at a time (it also replaces the scene's reset state)
        be.reset()
        be.sync()
        m = min(a.host_scenes, n)
        t0 = time.perf_counter()
        for i in range(m):
            got = be.load_scene(i, buf.copy())
            edited, _, _ = ref.add_ref(got, rows[i])
            be.write_scene(edited, i, 1)
        be.sync()
        host_us = (time.perf_counter() - t0) * 1e6
        t0 = time.perf_counter()
        for i in range(m):
            ref.add_ref(buf, rows[i])
        edit_us = (time.perf_counter() - t0) * 1e6
        result.update(
            what="BatchEngine.add_particles against load_scene + numpy edit + write_scene; reset and frame of scenes without a spawn "
                 "against the parent commit; reset and frame of scenes with the spawns",
            rows_per_scene=k, particles_added=added, add_particles_us=add, add_particles_skip_touching_us=skip,
            add_particles_kernel_vgprs=be.info("add_particles_kernel_vgprs"),
            host_route=dict(scenes_timed=m, total_us=host_us, per_scene_us=host_us / m, of_which_numpy_edit_us_per_scene=edit_us / m,
                            scaled_to_all_scenes_us=host_us / m * n,
                            scaling="linear in the scenes: the route handles one scene per call and waits for the stream twice per scene"),
            ratio_host_route_over_add_particles=host_us / m * n / add["median"],
            with_spawns=dict(frame_us=frame_after, reset_us=reset_after))
        if a.parent:
            with open(a.parent) as f:
                parent = json.load(f)
            result["parent_commit"] = dict(reset_us=parent["reset_us"], frame_us=parent["frame_us"], scenes=parent["scenes"], device=parent["device"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    be.destroy()


if __name__ == "__main__":
    main()
