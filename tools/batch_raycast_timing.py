"""What BatchEngine.raycast costs: 4096 default scenes, raycast at k = 16, 64 and 256 rays per scene (t, hit and
counts, all three masks, no limit on t), timed with HIP events on the batch's stream -- medians of 20 with the minimum and the
maximum -- beside one frame() of the same batch for scale and beside the route it replaces at k = 64: state_tensors() plus
graph()'s ends plus a torch broadcast of the same three tests over rays x (particles + beams), in chunks of scenes so that its
[chunk, k, max_particles + max_beams] temporaries fit (the chunk is recorded; that route gives distances only, knows nothing of
labels, and its minimum is not pinned bit for bit).  Then 256 scenes of 1024 particles / 4096 beams at k = 256.  The tool records
the numbers; it judges no ratio.
Usage: python tools/batch_raycast_timing.py --out profiles/batch_raycast_timing.json [--scenes 4096] [--repeats 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fan(torch, sb, n, k, seed):
    """k rays per scene: seeded origins inside the box, unit directions, no limit"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    origin = (torch.rand((n, k, 2), generator=g) * 1000.0).cuda()
    turn = torch.rand((n, k), generator=g) * (2.0 * np.pi)
    direction = torch.stack([torch.cos(turn), torch.sin(turn)], dim=2).cuda()
    return origin, direction, sb.batch.ray_rows(origin, direction, float("inf"))


def torch_route(torch, be, origin, direction, radius, bounds, chunk):
    """distances by broadcasting: what a caller writes today"""
    p, _, _ = be.state_tensors()
    ends = be.graph(counts=False).ends.to(torch.int64)
    inf = torch.tensor(float("inf"), device="cuda")
    out = []
    for s in range(0, be.n_scenes, chunk):
        pos, e, o, d = p[s:s + chunk, :, :2], ends[s:s + chunk], origin[s:s + chunk, :, None, :], direction[s:s + chunk, :, None, :]
        w = pos[:, None, :, :] - o                                   # [c, k, P, 2]
        a = (d * d).sum(-1)
        b = (w * d).sum(-1)
        c = (w * w).sum(-1) - radius * radius
        q = b * b - a * c
        t_disc = torch.where(c <= 0, torch.zeros_like(b), torch.where((b > 0) & (q >= 0), (b - q.clamp_min(0).sqrt()) / a, inf))
        live = (e[:, :, 0] >= 0)[:, None, :]
        idx = e.clamp_min(0)
        pa = torch.gather(pos, 1, idx[:, :, 0:1].expand(-1, -1, 2))[:, None]      # [c, 1, B, 2]
        pb = torch.gather(pos, 1, idx[:, :, 1:2].expand(-1, -1, 2))[:, None]
        ex, w = pb - pa, pa - o
        den = d[..., 0] * ex[..., 1] - d[..., 1] * ex[..., 0]
        tn = w[..., 0] * ex[..., 1] - w[..., 1] * ex[..., 0]
        un = w[..., 0] * d[..., 1] - w[..., 1] * d[..., 0]
        sgn = torch.sign(den)
        den, tn, un = den * sgn, tn * sgn, un * sgn
        t_seg = torch.where(live & (den > 0) & (un >= 0) & (un <= den) & (tn >= 0), tn / den, inf)
        o2, d2 = o[:, :, 0, :], d[:, :, 0, :]
        t_wall = torch.where(d2 < 0, (0.0 - o2) / d2, torch.where(d2 > 0, (bounds - o2) / d2, inf))
        t_wall = torch.where(t_wall >= 0, t_wall, inf).amin(-1)
        t_disc = torch.where(t_disc >= 0, t_disc, inf)                # (NaN rows of no particle: no hit)
        out.append(torch.minimum(torch.minimum(t_disc.amin(-1), t_seg.amin(-1)), t_wall))
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
    res = dict(what="BatchEngine.raycast against state_tensors() + a torch broadcast, and one frame for scale",
               device=torch.cuda.get_device_name(0), scenes=n, particles_per_scene=buf.particle_count, beams_per_scene=buf.beam_count,
               repeats=a.repeats, raycast_us={})
    for k in (16, 64, 256):
        origin, direction, rows = fan(torch, sb, n, k, k)
        t = torch.empty((n, k), dtype=torch.float32, device="cuda")
        hit = torch.empty((n, k, 3), dtype=torch.int32, device="cuda")
        counts = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        call = lambda: be.raycast(rows, t=t, hit=hit, counts=counts)
        call()
        be.sync()
        res["raycast_us"]["k=%d" % k] = timed(be, call)
        if k == 64:
            route = lambda: torch_route(torch, be, origin, direction, 10.0, 1000.0, a.chunk)
            far = route()
            torch.cuda.synchronize()
            call()
            be.sync()
            worst = float((far - t).abs().max())
            res["torch_route_k=64"] = dict(us=timed(be, route), chunk_scenes=a.chunk, max_abs_difference_to_raycast=worst,
                                           note="distances only; chunked over scenes so that [chunk, k, P + B] temporaries fit")
    be.frame()
    be.sync()
    res["frame_us"] = timed(be, lambda: be.frame())
    res["raycast_kernel_vgprs"], res["raycast_lds_bytes"] = be.info("raycast_kernel_vgprs"), be.info("raycast_lds_bytes")
    be.destroy()

    import batch_add_beams_cases as add_cases
    big = add_cases.big_scene(sb, 4096, 32)
    m = a.big_scenes
    be = sb.BatchEngine(n_scenes=m, layout=2, max_particles=1024, max_beams=4096, collision_mode=0)
    be.write_scene(big)
    _, _, rows = fan(torch, sb, m, 256, 1024)
    call = lambda: be.raycast(rows)
    call()
    be.sync()
    res["full_capacity"] = dict(scenes=m, particles_per_scene=1024, beams_per_scene=4096, k=256, raycast_us=timed(be, call),
                                raycast_lds_bytes=be.info("raycast_lds_bytes"))
    be.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
