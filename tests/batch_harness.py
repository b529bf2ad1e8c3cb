"""What the GPU tests of the batch share: making a BatchEngine for a case of tests/batch_cases.py (and of the modules built on it),
uploading its scenes, running the ops of its program, reading the scenes back.  A plain module, imported like batch_cases."""
import numpy as np

OFF, ALLPAIRS, GRID = 0, 1, 2


def make_batch(sb, case, n=None, mode=None, grid_min_particles=None):
    """n: scenes (None: one per buffer of the case); mode: the collision mode (None: GRID where the case collides, else OFF);
    bounds and radius are the case's own where it names them (batch_grid_cases), else the engine's 1000 / 10."""
    mode = (GRID if case["mode"] else OFF) if mode is None else mode
    return sb.BatchEngine(n_scenes=n or len(case["bufs"]), bounds_size=case.get("bounds", 1000.0), particle_radius=case.get("radius", 10.0),
                          layout=case["layout"], max_particles=case["cap"][0], max_beams=case["cap"][1], collision_mode=mode,
                          subticks=case.get("subticks", 64), grid_min_particles=grid_min_particles)


def upload_each(be, bufs):
    for i, b in enumerate(bufs):
        if b is not None:
            be.write_scene(b, i, 1)


def device_bytes(rows):
    import torch
    a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), 32).copy()
    return torch.from_numpy(a).cuda()


def apply_to_batch(be, op):
    if op[0] == "frame":
        be.frame(op[1])
    elif op[0] == "step":
        be.step(op[1])
    elif op[0] == "delete":
        be.delete_pass()
    elif op[0] == "consts":
        be.set_physics_constants(op[2], first=op[1], count=1)
    elif op[0] == "input":
        be.write_user_input(op[1])
    elif op[0] == "inputs":
        be.write_user_input(device_bytes(op[1]))
    else:
        raise ValueError(op)


def load_all(be, bufs):
    return [None if b is None else be.load_scene(i, b.copy()) for i, b in enumerate(bufs)]
