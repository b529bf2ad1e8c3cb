"""What the free-index allocator of BatchEngine.add_beams / add_particles costs at full width: scenes of capacity
1024 particles / 4096 beams -- bitmaps of 32 and 128 words, the widest the prefix ever scans -- holding the default scene, 8 rows
per scene, each call timed with HIP events on the batch's stream after a reset() (medians of --repeats).  Run it from the checkout
to measure; tools/batch_add_beams_timing.py and tools/batch_add_particles_timing.py time the same calls at capacity 128 / 320.
Usage: python tools/batch_alloc_timing.py --out width.json [--scenes 1024] [--repeats 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--scenes", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    sb = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    import batch_add_beams_ref as beam_ref
    import batch_add_particles_ref as part_ref
    n, k = a.scenes, 8
    buf = sb.scenes.default_buffers(1, 1024, 4096)
    be = sb.BatchEngine(n_scenes=n, max_particles=1024, max_beams=4096)
    be.write_scene(buf)
    stream = torch.cuda.ExternalStream(be.stream())
    pd = buf.mapping[:buf.particle_count].astype(int)
    welds = beam_ref.pack([(int(pd[j]), int(pd[j + 40]), 30.0, 1.0, 50.0, 1.0, 2.5) for j in range(k)])
    spawns = part_ref.pack([(0, 300.0 + 40.0 * j, 300.0) for j in range(k)])
    dw, ds = (torch.from_numpy(np.stack([r] * n)).cuda() for r in (welds, spawns))
    res = torch.empty((n, k), dtype=torch.int32, device="cuda")
    cnt = torch.empty((n, 4), dtype=torch.int32, device="cuda")

    def timed(fn):
        out = []
        for _ in range(a.repeats + 1):      # (the first run warms)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                be.reset()
                be.sync()
                e0.record()
                fn()
                e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1000.0)
        out = out[1:]
        return dict(median=float(np.median(out)), min=float(np.min(out)), max=float(np.max(out)))

    result = dict(device=torch.cuda.get_device_name(0), scenes=n, capacity=[1024, 4096], rows_per_scene=k, repeats=a.repeats,
                  add_beams_us=timed(lambda: be.add_beams(dw, result=res, counts=cnt)),
                  add_particles_us=timed(lambda: be.add_particles(ds, result=res, counts=cnt)))
    result["added"] = int(cnt[:, 0].sum().item())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    be.destroy()


if __name__ == "__main__":
    main()
