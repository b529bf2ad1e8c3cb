"""BatchEngine.contacts beside one frame() of the same batch and beside the export route.

    python tools/batch_contacts_timing.py [--repeats 25] [--out profiles/batch_contacts_timing.json]

All times are HIP events on the batch's stream (torch's current stream is made the batch's for the whole run, so the torch half of
the export route is in the same queue), warm, median of --repeats.
Shapes: 4096 default scenes (119 / 299) at capacity 128 / 320 after 3 frames; 4096 lattices of 32 x 32 (1024 / 2945) at capacity
1024 / 4096 after 3 frames.

  contacts        contacts(touch=, counts=) into preallocated tensors, no labels, no pair list
  contacts_pairs  the same with a pair list of PAIRS rows per scene
  contacts_bodies contacts(labels=True, pairs=): bodies() first, then the call with its labels
  frame           frame(1)
  export          state_tensors() plus, in chunks of CHUNK scenes, torch.cdist of the positions and `< 2r` on it, summed per particle:
                  the route a user has without the call (it cannot reproduce the engine's test at the boundary and lists no pairs)
The expectation: contacts() costs less than one frame() of the same batch, in both shapes."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_timing_shapes import scene  # noqa: E402

SHAPES = {"default_4096": (4096, 128, 320, 1, "default"), "lattice_32x32_4096": (4096, 1024, 4096, 2, "lattice")}
PAIRS = 256
CHUNK = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    sb = __import__("__graft_entry__").load_package()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0),
           "protocol": "HIP events on the batch's stream, warm, median of %d; both shapes after 3 frames" % a.repeats, "shapes": {}}
    for name, (n, maxp, maxb, layout, kind) in SHAPES.items():
        buf = scene(sb, kind, layout, maxp, maxb)
        be = sb.BatchEngine(n_scenes=n, layout=layout, max_particles=maxp, max_beams=maxb)
        be.write_scene(buf)
        be.frame(3)
        stream = torch.cuda.ExternalStream(be.stream(), device=dev)
        two_r = 20.0

        def timed(call):
            ms = []
            for k in range(a.warmup + a.repeats):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                call()
                t1.record(stream)
                t1.synchronize()
                if k >= a.warmup:
                    ms.append(t0.elapsed_time(t1))
            return {"ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}

        with torch.cuda.stream(stream):
            touch = torch.empty((n, maxp, 4), dtype=torch.int32, device=dev)
            counts = torch.empty((n, 4), dtype=torch.int32, device=dev)
            pairs = torch.empty((n, PAIRS, 2), dtype=torch.int32, device=dev)

            def export():
                p, _, _ = be.state_tensors()
                out = torch.empty((n, maxp), dtype=torch.int32, device=dev)
                for s in range(0, n, CHUNK):
                    xy = p[s:s + CHUNK, :, :2]
                    out[s:s + CHUNK] = (torch.cdist(xy, xy) < two_r).sum(dim=2, dtype=torch.int32) - 1   # (NaN rows: no particle, -1)
                return out

            r = {"contacts": timed(lambda: be.contacts(touch=touch, counts=counts)),
                 "contacts_pairs": timed(lambda: be.contacts(touch=touch, counts=counts, pairs=pairs)),
                 "contacts_bodies": timed(lambda: be.contacts(labels=True, touch=touch, counts=counts, pairs=pairs)),
                 "export": timed(export)}
            be.contacts(touch=touch, counts=counts, pairs=pairs)
            stream.synchronize()
            r["counts_row_0"] = counts[0].tolist()
            r["all_rows_equal"] = bool((counts == counts[0]).all())
            r["max_pairs_in_a_scene"] = int(counts[:, 0].max())
            r["frame"] = timed(lambda: be.frame(1))    # (last: it moves the scenes on)
        r["kernel"] = {x: be.info(x) for x in ("contacts_kernel_vgprs", "contacts_kernel_scratch_bytes", "contacts_lds_bytes", "contacts_cells_per_side")}
        r.update(n_scenes=n, capacity=[maxp, maxb], particles_beams=[buf.particle_count, buf.beam_count], pair_list_rows=PAIRS,
                 contacts_over_frame=r["contacts"]["ms"] / r["frame"]["ms"], contacts_pairs_over_frame=r["contacts_pairs"]["ms"] / r["frame"]["ms"],
                 export_over_contacts=r["export"]["ms"] / r["contacts"]["ms"],
                 cheaper_than_a_frame=max(r["contacts"]["max_ms"], r["contacts_pairs"]["max_ms"]) < r["frame"]["min_ms"])
        res["shapes"][name] = r
        be.sync()
        be.destroy()
        print(name, {c: round(v["ms"], 4) for c, v in r.items() if isinstance(v, dict) and "ms" in v}, flush=True)
    res["expectation"] = "contacts(), with and without a pair list, costs less than one frame() of the same batch (every sample below every sample)"
    res["expectation_met"] = all(s["cheaper_than_a_frame"] for s in res["shapes"].values())
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
