"""What tests/test_gpu_fork.py runs (BatchEngine.fork / checkpoint / write_beams_device), on the ORACLE's side:
the scenes, the edits and the bookkeeping that says which oracle a scene follows after a fork.  tests/test_batch_fork_cpu.py runs
every program here through the oracle alone and asserts that it stays finite; the GPU tests compare bit for bit.
"""
import numpy as np

import batch_cases as bc

KEEP = 0xFFFFFFFF
ORACLE_ARRAYS = ("metadata", "mapping", "particles_a", "particles_b", "beams", "forces", "delete")


def clone(ref):
    """A second oracle in the same state, pending break flags (`delete`) and force sums included."""
    new = type(ref).__new__(type(ref))
    new.__dict__.update(ref.__dict__)
    for k in ORACLE_ARRAYS:
        setattr(new, k, getattr(ref, k).copy())
    return new


def is_finite(ref):
    return bool(np.isfinite(ref.particles_b if ref.final_in_b else ref.particles_a).all())


def fork_oracles(refs, src, constants=False):
    """The oracles after fork(src): scene i follows a clone of OLD oracle src[i] that keeps scene i's user input and (unless
    constants) scene i's physics constants.  Entries equal to i, KEEP or outside the batch leave the oracle as it is; None is a
    scene never uploaded (its metadata words are zero, so only constants=True gives it physics constants worth stepping with)."""
    out = []
    for i, s in enumerate(src):
        s = int(s) & 0xFFFFFFFF
        if s == i or s >= len(refs):
            out.append(refs[i])
        elif refs[s] is None:
            out.append(None)
        else:
            new = clone(refs[s])
            if refs[i] is not None:
                new.metadata[20:28] = refs[i].metadata[20:28]
                if not constants:
                    new.metadata[12:20] = refs[i].metadata[12:20]
            else:
                assert constants, "a never-uploaded destination has all-zero physics constants"
                new.metadata[20:28] = 0
            out.append(new)
    return out


def fork_templates(templates, src):
    """load_scene writes only what the scene's upload reaches, so scene i is read into a copy of its SOURCE's upload."""
    n = len(templates)
    return [templates[i] if (int(s) & 0xFFFFFFFF) == i or (int(s) & 0xFFFFFFFF) >= n else templates[int(s) & 0xFFFFFFFF]
            for i, s in enumerate(src)]


def advance(refs, ops):
    for op in ops:
        bc.apply_to_oracles(refs, op)


# ---------------------------------------------------------------- scenes made distinct by their user input
def distinct_inputs(sb, n):
    """One 32-byte user input per scene: different applied forces, every fifth scene with the mouse grab active."""
    out = []
    for i in range(n):
        b = sb.Buffers(1, 4, 4)
        b.user_strength = 1.0 + 0.125 * (i % 7)
        b.set_user_input(applied_force=(0.02 * (i % 9) - 0.08, 0.015 * (i % 5)), mouse_pos=(200.0 + 9.0 * i, 150.0 + 3.0 * i),
                         mouse_vel=(3.0, 1.0), mouse_active=(i % 5 == 4))
        out.append(b.user_input_bytes())
    return out


def case_distinct(sb, n):
    """n default scenes (128 / 320, v1), each with its own user input, one frame: n different states."""
    buf = sb.scenes.default_buffers(1, 128, 320)
    return dict(name="default scene x %d, distinct inputs" % n, layout=1, cap=(128, 320), mode=bc.ALLPAIRS, bufs=[buf] * n,
                program=[("inputs", distinct_inputs(sb, n)), ("frame", 1)])


def snapshot_sources(n):
    """(name, src) of the snapshot test, applied one after the other with a frame in between."""
    rot = [(i + 1) % n for i in range(n)]
    swap = list(range(n))
    swap[3], swap[n - 2] = n - 2, 3
    bcast = [1] + [0] * (n - 1)              # scene 0, everybody's source, is itself overwritten (by scene 1)
    return [("rotation", rot), ("swap", swap), ("broadcast of an overwritten scene", bcast)]


KEEP_SOURCES = [KEEP, 1, 8, 0x7FFFFFFF, 0, 5, KEEP, 2]      # N = 8: scenes 4 and 7 change, two entries name no scene
KEEP_BAD = 2

CONSTS4 = [[0.0, -0.5, 0.5, 0.2, 0.5, 0.1, 0.001, 2.0], [0.1, -0.8, 0.4, 0.3, 0.6, 0.2, 0.002, 2.0],
           [-0.05, -0.3, 0.6, 0.1, 0.4, 0.05, 0.0005, 3.0], [0.0, -1.0, 0.3, 0.25, 0.7, 0.15, 0.002, 2.5]]
CONSTS_SOURCES = [1, 0, 3, 2]


def case_consts(sb):
    """batch_cases.case_inputs' four scenes with different physics constants as well."""
    buf = sb.scenes.default_buffers(1, 128, 320)
    return dict(name="constants and input", layout=1, cap=(128, 320), mode=bc.ALLPAIRS, bufs=[buf] * 4,
                program=[("consts", i, np.array(c, "f4")) for i, c in enumerate(CONSTS4)] + [("inputs", bc.user_inputs(sb, 0)), ("frame", 1)])


# ---------------------------------------------------------------- beam import
def beam_case(sb, n=4):
    return case_distinct(sb, n)


def beam_factors(n, max_beams):
    """float32 [n, max_beams]: 1 outside a subset (every third data index), 0.8 .. 1.2 inside, different per scene and beam."""
    idx = np.arange(max_beams)
    f = np.ones((n, max_beams), "f4")
    for s in range(n):
        k = (idx * 7 + s * 3) % 11
        f[s] = np.where(idx % 3 == 0, np.float32(0.8) + np.float32(0.04) * k.astype("f4"), np.float32(1.0))
    return f


LAST_FACTOR = np.float32(1.0 + 1.0 / 256.0)        # last_length of the subset, scaled a little (it only feeds the damping term)
BEAM_ROUNDS = [(True, False), (False, True), (True, True)]      # (target_length, last_length) of write_beams_device, a frame after each


def edit_beams(export, factors, target, last):
    """The edit of one round on an export [n, max_beams, 4] (numpy float32; rows of no beam are NaN and stay so)."""
    out = export.copy()
    if target:
        out[:, :, 0] = export[:, :, 0] * factors
    if last:
        out[:, :, 1] = export[:, :, 1] * np.where(factors != 1.0, LAST_FACTOR, np.float32(1.0)).astype("f4")
    return out


def export_of(ref, template):
    """What read_state_device gives for an oracle's beams: [max_beams, 4] float32, NaN where the upload has no beam."""
    out = np.full((template.max_beams, 4), np.nan, "f4")
    idx = template.mapping[template.max_particles:template.max_particles + template.beam_count].astype(np.int64)
    for k, f in enumerate(("target_length", "last_length", "strain", "stress")):
        out[idx, k] = ref.beams[f][idx]
    return out


def import_into_oracle(ref, template, rows, target, last):
    """The same float32 values into the oracle's beam buffer through load_buffers -> write_buffers (at a frame boundary, where
    that round trip is bit-neutral: test_batch_fork_cpu.py)."""
    buf = ref.load_buffers(template.copy())
    idx = template.mapping[template.max_particles:template.max_particles + template.beam_count].astype(np.int64)
    if target:
        buf.beams["target_length"][idx] = rows[idx, 0]
    if last:
        buf.beams["last_length"][idx] = rows[idx, 1]
    ref.write_buffers(buf)
