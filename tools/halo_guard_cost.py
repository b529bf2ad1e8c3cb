"""What does the halo guard cost in the real refresh loop?  (include/softbody.h sb_halo_guard)

BASELINE config 4's share at depth 24: an interior 500 x 4000 slab (two neighbours, 2 x 24 ghost columns), collisions off
(config 4), so the guard runs checks (C) and (D).  There are no neighbours on one GPU, so every refresh hands each ghost
record its own current value (sb_halo_configure with the ghost lists as the send lists too: pack the ghosts, unpack them
again).  The ghost zone then evolves as a lattice with a free outer edge: nothing stretches, and the guard must stay silent
(`guard_fired` == "") -- the cost of a guard that finds nothing, the case that matters (H and s: below).  The loop -- `depth` substeps, one
refresh (pack, unpack and, when on, the guard behind it), repeated -- is timed with the guard off and on, alternately.
Writes one JSON record to argv[1] (default: stdout only)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

sb = ge.load_package()
W, H, DEPTH, PERIODS, ROUNDS = 500, 4000, 24, 40, 7
buf, plan = sb.halo.slab_scene(sb, 1, 3, W, H, d=30.0, origin=(1000.0, 1000.0), jitter=1.0, depth=DEPTH)
eng = sb.Engine(bounds_size=float(max(3 * W, H) * 30 + 2000), layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams,
                collision_mode=0)
eng.write_buffers(buf)
gp, _, gb, _ = plan.lists()
eng.halo_configure(gp, gp, gb, gb)                 # every ghost record is sent to itself: a refresh that changes nothing
packed = torch.zeros(6 * gp.size + 2 * gb.size, device="cuda")


def refresh():
    eng.halo_pack(packed.data_ptr())
    eng.halo_unpack(packed.data_ptr())


own = plan.owned_particles
x = buf.particles[own, 0]
lo = np.array([x.min() - W * 30.0, x.min(), x.max() + 30.0], "<f4")      # (unused by checks C and D)
hi = np.array([x.min() - 30.0, x.max(), x.max() + W * 30.0], "<f4")
# H = 3 x the longest beam and s = 1 unit per substep: the slab falls and lands, and a run at the default allowance
# (H = 1.5 x, s = H / 16D = 0.18 per substep) sees (D) fire on the landing; a firing guard costs other bytes than a silent one
hop, motion = 3.0 * (30.0 * 2 ** 0.5 + 3.0), 1.0
ext = torch.cuda.ExternalStream(eng.stream(), device=torch.device("cuda", 0))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def loop_us():
    for _ in range(2):
        eng.step(DEPTH)
        refresh()
    eng.sync()
    with torch.cuda.stream(ext):
        e0.record()
    for _ in range(PERIODS):
        eng.step(DEPTH)
        refresh()
    with torch.cuda.stream(ext):
        e1.record()
    eng.sync()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (PERIODS * DEPTH)


off, on, fired = [], [], []
for _ in range(ROUNDS):
    eng.halo_guard_off()
    off.append(loop_us())
    eng.halo_guard(1, 3, DEPTH, 0.0, hop, lo, hi, own, np.zeros(own.size, "<u8"), plan.owned_beams, motion)
    on.append(loop_us())
    status = eng.halo_guard_status()
    fired.append(status.kind_names)
rec = dict(tool="tools/halo_guard_cost.py", scene="config 4 share: interior slab %d x %d (+2 x %d ghost columns), collisions off, "
           "ghosts refreshed with their own values" % (W, H, DEPTH),
           depth=DEPTH, hop=hop, motion=motion, periods_per_round=PERIODS, rounds=ROUNDS, own_particles=int(own.size), own_beams=int(plan.owned_beams.size),
           us_per_substep_guard_off=off, us_per_substep_guard_on=on,
           median_off=float(np.median(off)), median_on=float(np.median(on)),
           overhead_pct=float(100.0 * (np.median(on) / np.median(off) - 1.0)), target_pct=2.0,
           guard_fired="".join(sorted(set("".join(fired)))), guard_refreshes_per_round=status.refreshes)
eng.destroy()
print(json.dumps(rec))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1)
