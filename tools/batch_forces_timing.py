"""What BatchEngine.forces costs: on 4096 default scenes and on 256 scenes of 1024 particles / 4096 beams, timed with
HIP events on the batch's stream -- medians of 20 with the minimum and the maximum, microseconds -- forces() (rows, tension and
counts), forces(labels=True, other_body=True), contacts() and summary() on the same batch (the two existing reports with the same
loads), one frame(), and the route forces() replaces: state_tensors() plus graph(material=True) plus a torch restatement of the
beam force alone (no fixed point, no saturation, no contacts).  With --parent-root DIR, a checkout of the parent commit (its
library is built there if missing), frame() of the parent is timed in a child process of the same job: stepping must cost what it
did.  Without --parent-root that comparison is NOT made: parent_frame_us is null and a warning goes to stderr.  The tool records
the numbers; it judges no ratio.
Usage: python tools/batch_forces_timing.py --out profiles/batch_forces_timing.json [--parent-root DIR] [--repeats 20]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np


def load(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(root, "softbody-webgpu_amd", "csrc", "libsoftbody_hip.so")):
        ge.build()
    return ge.load_package()


def torch_beam_force(torch, be):
    """what a caller writes today: per-beam force vectors from the exported state, summed per particle with index_add_"""
    p, b, alive = be.state_tensors()
    g = be.graph(material=True, counts=False)
    ends, mat = g.ends.to(torch.int64).clamp_min(0), g.material
    live = (g.ends[..., 0] >= 0)
    pos = p[..., :2].nan_to_num(0.0)
    pa = torch.gather(pos, 1, ends[..., 0:1].expand(-1, -1, 2))
    pb = torch.gather(pos, 1, ends[..., 1:2].expand(-1, -1, 2))
    d = pb - pa
    length = d.norm(dim=-1).clamp_min(1e-10)
    mag = (b[..., 0] - length) * mat[..., 1] + (b[..., 1] - length) * mat[..., 2]
    f = torch.where(live[..., None], d / length[..., None] * mag[..., None], torch.zeros_like(d))
    out = torch.zeros_like(pos)
    out.scatter_add_(1, ends[..., 1:2].expand(-1, -1, 2), f)
    out.scatter_add_(1, ends[..., 0:1].expand(-1, -1, 2), -f)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--parent-root")
    ap.add_argument("--frame-only", action="store_true", help="(the child process of --parent-root: frame() alone, JSON on stdout)")
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--big-scenes", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import torch
    sb = load(a.root)
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")

    def timed(be, fn):
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

    def shapes():
        yield "default", a.scenes, sb.scenes.default_buffers(1, 128, 320), dict(max_particles=128, max_beams=320)
        lat = sb.scenes.lattice_buffers(32, 32, d=19.0, origin=(100.0, 100.0), spring=50.0, damp=700.0, yield_strain=0.2, strain_limit=0.5, jitter=1.5,
                                        layout=2)
        big = sb.Buffers(2, 1024, 4096)
        big.set_scene(lat.particles[:1024], lat.beams[:lat.beam_count].copy())
        yield "full_capacity", a.big_scenes, big, dict(layout=2, max_particles=1024, max_beams=4096)

    res = dict(what="BatchEngine.forces beside contacts(), summary(), one frame() and the export route; microseconds", device=torch.cuda.get_device_name(0),
               repeats=a.repeats)
    for name, n, buf, kw in shapes():
        be = sb.BatchEngine(n_scenes=n, **kw)
        be.write_scene(buf)
        be.frame()
        be.sync()
        r = dict(scenes=n, particles_per_scene=buf.particle_count, beams_per_scene=buf.beam_count, frame_us=timed(be, lambda: be.frame()))
        if not a.frame_only:
            rows = torch.empty((n, be.max_particles, 8), dtype=torch.float32, device="cuda")
            tension = torch.empty((n, be.max_beams), dtype=torch.float32, device="cuda")
            counts = torch.empty((n, 4), dtype=torch.int32, device="cuda")
            touch = torch.empty((n, be.max_particles, 4), dtype=torch.int32, device="cuda")
            summ = torch.empty((n, 24), dtype=torch.float32, device="cuda")
            labels = be.bodies()[0]
            for key, fn in (("forces_us", lambda: be.forces(rows=rows, tension=tension, counts=counts)),
                            ("forces_other_body_us", lambda: be.forces(labels=True, other_body=True, rows=rows, tension=tension, counts=counts)),
                            ("forces_other_body_given_labels_us", lambda: be.forces(labels=labels, other_body=True, rows=rows, tension=tension, counts=counts)),
                            ("contacts_us", lambda: be.contacts(touch=touch, counts=counts)), ("summary_us", lambda: be.summary(out=summ)),
                            ("export_route_us", lambda: torch_beam_force(torch, be))):
                fn()
                be.sync()
                torch.cuda.synchronize()
                r[key] = timed(be, fn)
            r["forces_kernel_vgprs"], r["forces_lds_bytes"] = be.info("forces_kernel_vgprs"), be.info("forces_lds_bytes")
        be.destroy()
        res[name] = r
    if a.frame_only:
        print(json.dumps(res))
        return
    if a.parent_root:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--frame-only", "--root", os.path.abspath(a.parent_root), "--scenes", str(a.scenes),
                            "--big-scenes", str(a.big_scenes), "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit("the parent's frame() could not be timed: " + p.stderr[-2000:])
        parent = json.loads(p.stdout.strip().splitlines()[-1])
        res["parent_frame_us"] = {k: parent[k]["frame_us"] for k in ("default", "full_capacity")}
    else:
        res["parent_frame_us"] = None
        print("warning: no --parent-root: the parent commit's frame() was not timed, so this run does not show that stepping costs what it did",
              file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
