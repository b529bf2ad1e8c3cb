"""What BatchEngine.nearest costs: 4096 default scenes, nearest at k = 16, 64 and 256 points per scene (d, hit, point,
within and counts, all three masks, a reach of 100), timed with HIP events on the batch's stream -- medians of 20 with the minimum
and the maximum -- beside raycast() at the same k and one frame() of the same batch for scale, and beside the route it replaces at
k = 64: state_tensors() plus graph()'s ends plus a torch clamp-projection broadcast over points x (particles + beams), in chunks of
scenes so that its [chunk, k, max_particles + max_beams] temporaries fit (the chunk is recorded; that route gives distances only,
knows nothing of labels, ties or counts, and its minimum is not pinned bit for bit).  Then 256 scenes of 1024 particles / 4096 beams
at k = 256.  The tool records the numbers; it judges no ratio.
Usage: python tools/batch_nearest_timing.py --out profiles/batch_nearest_timing.json [--scenes 4096] [--repeats 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REACH = 100.0


def probes(torch, sb, n, k, seed):
    """k points per scene: seeded inside the box; the rows of nearest() and, from the same points, a fan of rays for raycast()"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    point = (torch.rand((n, k, 2), generator=g) * 1000.0).cuda()
    turn = torch.rand((n, k), generator=g) * (2.0 * np.pi)
    direction = torch.stack([torch.cos(turn), torch.sin(turn)], dim=2).cuda()
    rows = sb.batch.point_rows(point, REACH) if hasattr(sb.batch, "point_rows") else None   # (None: a build without nearest())
    return point, rows, sb.batch.ray_rows(point, direction, float("inf"))


def torch_route(torch, be, point, bounds, chunk):
    """distances by broadcasting: what a caller writes today"""
    p, _, _ = be.state_tensors()
    ends = be.graph(counts=False).ends.to(torch.int64)
    inf = torch.tensor(float("inf"), device="cuda")
    out = []
    for s in range(0, be.n_scenes, chunk):
        pos, e, o = p[s:s + chunk, :, :2], ends[s:s + chunk], point[s:s + chunk, :, None, :]
        v = pos[:, None, :, :] - o                                   # [c, k, P, 2]
        d2_p = (v * v).sum(-1)
        d2_p = torch.where(d2_p >= 0, d2_p, inf)                      # (NaN rows of no particle: nothing there)
        live = (e[:, :, 0] >= 0)[:, None, :]
        idx = e.clamp_min(0)
        pa = torch.gather(pos, 1, idx[:, :, 0:1].expand(-1, -1, 2))[:, None]      # [c, 1, B, 2]
        pb = torch.gather(pos, 1, idx[:, :, 1:2].expand(-1, -1, 2))[:, None]
        ex, w = pb - pa, o - pa
        ee, we = (ex * ex).sum(-1), (w * ex).sum(-1)
        u = (we / ee.clamp_min(1e-30)).clamp(0.0, 1.0)
        v = pa + u[..., None] * ex - o
        d2_b = torch.where(live, (v * v).sum(-1), inf)
        o2 = o[:, :, 0, :]
        d2_w = torch.minimum(o2, bounds - o2).amin(-1) ** 2
        out.append(torch.minimum(torch.minimum(d2_p.amin(-1), d2_b.amin(-1)), d2_w).sqrt())
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--big-scenes", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    sb = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")

    def timed(be, fn):
        """median, minimum and maximum of `repeats` runs of fn between two events on the batch's stream, in microseconds"""
        stream = torch.cuda.ExternalStream(be.stream())
        out = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            be.sync()
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                e0.record()
                fn()
                e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1000.0)
        return dict(median=float(np.median(out)), min=float(np.min(out)), max=float(np.max(out)))

    n = a.scenes
    buf = sb.scenes.default_buffers(1, 128, 320)
    be = sb.BatchEngine(n_scenes=n, max_particles=128, max_beams=320)
    be.write_scene(buf)
    res = dict(what="BatchEngine.nearest against state_tensors() + a torch broadcast, beside raycast at the same k and one frame for scale",
               device=torch.cuda.get_device_name(0), scenes=n, particles_per_scene=buf.particle_count, beams_per_scene=buf.beam_count,
               repeats=a.repeats, reach=REACH, nearest_us={}, raycast_us={})
    has_nearest = hasattr(be, "nearest")    # (the same tool times a build without it: frame and raycast only)
    for k in (16, 64, 256):
        point, rows, rays = probes(torch, sb, n, k, k)
        d = torch.empty((n, k), dtype=torch.float32, device="cuda")
        hit = torch.empty((n, k, 3), dtype=torch.int32, device="cuda")
        q = torch.empty((n, k, 2), dtype=torch.float32, device="cuda")
        within = torch.empty((n, k, 2), dtype=torch.int32, device="cuda")
        counts = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        cast = lambda: be.raycast(rays, t=d, hit=hit, counts=counts)
        cast()
        be.sync()
        res["raycast_us"]["k=%d" % k] = timed(be, cast)
        if not has_nearest:
            continue
        call = lambda: be.nearest(rows, d=d, hit=hit, point=q, within=within, counts=counts)
        call()
        be.sync()
        res["nearest_us"]["k=%d" % k] = timed(be, call)
        if k == 64:
            route = lambda: torch_route(torch, be, point, 1000.0, a.chunk)
            far = route()
            torch.cuda.synchronize()
            call()
            be.sync()
            found = hit[:, :, 0] > 0
            worst = float((far - d)[found].abs().max())
            res["torch_route_k=64"] = dict(us=timed(be, route), chunk_scenes=a.chunk, max_abs_difference_to_nearest=worst,
                                           note="distances only; chunked over scenes so that [chunk, k, P + B] temporaries fit")
    be.frame()
    be.sync()
    res["frame_us"] = timed(be, lambda: be.frame())
    if has_nearest:
        res["nearest_kernel_vgprs"], res["nearest_lds_bytes"] = be.info("nearest_kernel_vgprs"), be.info("nearest_lds_bytes")
    be.destroy()
    if not has_nearest:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
        return

    import batch_add_beams_cases as add_cases
    big = add_cases.big_scene(sb, 4096, 32)
    m = a.big_scenes
    be = sb.BatchEngine(n_scenes=m, layout=2, max_particles=1024, max_beams=4096, collision_mode=0)
    be.write_scene(big)
    _, rows, rays = probes(torch, sb, m, 256, 1024)
    call, cast = (lambda: be.nearest(rows)), (lambda: be.raycast(rays))
    call()
    cast()
    be.sync()
    res["full_capacity"] = dict(scenes=m, particles_per_scene=1024, beams_per_scene=4096, k=256, nearest_us=timed(be, call),
                                raycast_us=timed(be, cast), nearest_lds_bytes=be.info("nearest_lds_bytes"))
    be.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
