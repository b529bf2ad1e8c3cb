"""What BatchEngine.graph and Engine.graph cost: 4096 default scenes, graph(adjacency=True) -- ends, row_ptr, nbr and counts --
and graph() -- ends and counts alone (no sort: the degrees are an LDS histogram) -- timed with HIP events on the batch's stream, against the route they replace: load_scene
of every scene plus the numpy decode of tests/graph_ref.py, timed with the host clock over 64 scenes of the same batch in the same
process and scaled linearly to all scenes (the route is one scene per call, each with a wait for the stream, so its cost is per
scene); and one frame() beside them for scale; then the engine analogue at config 2 against
sb_load_buffers plus the same decode.  The tool records the numbers; it judges no ratio.
Usage: python tools/batch_graph_timing.py --out profiles/batch_graph_timing.json [--scenes 4096] [--repeats 20]"""
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
    ap.add_argument("--host-scenes", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    import graph_ref as ref
    ge.build()
    sb = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    n = a.scenes
    buf = sb.scenes.default_buffers(1, 128, 320)
    be = sb.BatchEngine(n_scenes=n, max_particles=128, max_beams=320)
    be.write_scene(buf)
    stream = torch.cuda.ExternalStream(be.stream())
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
    ends, row_ptr, nbr, counts = i32(n, 320, 2), i32(n, 129), i32(n, 640, 2), i32(n, 4)

    def timed(fn):
        """median and minimum of `repeats` runs of fn between two events on the batch's stream, in microseconds"""
        out = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            be.sync()
            with torch.cuda.stream(stream):
                e0.record()
                fn()
                e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1000.0)
        return dict(median=float(np.median(out)), min=float(np.min(out)))

    def adjacency():
        be.graph(ends=ends, adjacency=(row_ptr, nbr), counts=counts)

    def edges():
        be.graph(ends=ends, counts=counts)

    with torch.cuda.stream(stream):   # warm
        adjacency()
        edges()
        be.frame()
    be.sync()
    be.reset()
    t_adj, t_edges = timed(adjacency), timed(edges)
    t_frame = timed(lambda: be.frame())
    be.reset()
    be.sync()
    adjacency()
    be.sync()
    got = ref.Graph(ends[0].cpu().numpy(), None, row_ptr[0].cpu().numpy(), nbr[0].cpu().numpy(), counts[0].cpu().numpy())
    # the host route, one scene at a time
    m = min(a.host_scenes, n)
    t0 = time.perf_counter()
    for i in range(m):
        want = ref.graph_ref(be.load_scene(i, buf.copy()))
    host_us = (time.perf_counter() - t0) * 1e6
    t0 = time.perf_counter()
    for i in range(m):
        ref.graph_ref(buf)
    decode_us = (time.perf_counter() - t0) * 1e6
    if ref.same(got, want):
        raise SystemExit("graph() differs from the host route in %s: nothing is recorded" % ref.same(got, want))
    result = dict(
        what="BatchEngine.graph against load_scene + a numpy decode per scene, and one frame for scale",
        device=torch.cuda.get_device_name(0), scenes=n, particles_per_scene=buf.particle_count, beams_per_scene=buf.beam_count,
        repeats=a.repeats, graph_adjacency_us=t_adj, graph_ends_counts_us=t_edges, frame_us=t_frame,
        graph_kernel_vgprs=be.info("graph_kernel_vgprs"), graph_lds_bytes=be.info("graph_lds_bytes"),
        host_route=dict(scenes_timed=m, total_us=host_us, per_scene_us=host_us / m, of_which_numpy_decode_us_per_scene=decode_us / m,
                        scaled_to_all_scenes_us=host_us / m * n,
                        scaling="linear in the scenes: the route handles one scene per call and waits for the stream every time"),
        engine=engine_timing(sb, ref, a.repeats))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    be.destroy()


def engine_timing(sb, ref, repeats):
    """the engine analogue at config 2 (a 1000 x 1000 lattice): Engine.graph(adjacency=True) by HIP events on the engine's stream
    against sb_load_buffers plus the numpy decode, the host clock, once"""
    import torch
    buf = sb.scenes.lattice_buffers(1000, 1000, d=30.0, jitter=1.0, layout=2)
    eng = sb.Engine(bounds_size=40000.0, layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=0)
    eng.write_buffers(buf)
    stream = torch.cuda.ExternalStream(eng.stream())
    i32, i64 = (lambda *sh: torch.empty(sh, dtype=torch.int32, device="cuda")), (lambda *sh: torch.empty(sh, dtype=torch.int64, device="cuda"))
    ends, row_ptr, nbr, counts = i32(eng.max_beams, 2), i64(eng.max_particles + 1), i32(2 * eng.max_beams, 2), i64(4)
    call = lambda: eng.graph(ends=ends, adjacency=(row_ptr, nbr), counts=counts)
    call()                                      # (builds the tables)
    eng.sync()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        with torch.cuda.stream(stream):
            e0.record()
            call()
            e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0)
    t0 = time.perf_counter()
    now = eng.load_buffers(buf.copy())
    t1 = time.perf_counter()
    want = ref.graph_ref(now)
    t2 = time.perf_counter()
    ok = bool(np.array_equal(ends.cpu().numpy(), want.ends) and np.array_equal(row_ptr.cpu().numpy(), want.row_ptr) and
              np.array_equal(nbr.cpu().numpy(), want.nbr) and np.array_equal(counts.cpu().numpy(), want.counts))
    res = dict(scene="config 2: 1000 x 1000 lattice", particles=buf.particle_count, beams=buf.beam_count, equals_host_route=ok,
               graph_adjacency_us=dict(median=float(np.median(out)), min=float(np.min(out))), table_build_us=eng.info("graph_table_build_us"),
               host_route=dict(load_buffers_us=(t1 - t0) * 1e6, numpy_decode_us=(t2 - t1) * 1e6, total_us=(t2 - t0) * 1e6))
    eng.destroy()
    return res


if __name__ == "__main__":
    main()
