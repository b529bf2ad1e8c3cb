"""The hand-built scenes of tests/test_graph_cpu.py and tests/test_gpu_batch_graph.py (BatchEngine.graph)."""
import numpy as np

MAT = (50.0, 700.0, 0.2, 1.0e9)        # spring, damp, yield_strain, strain_break_limit
CORNER_CAP = (1024, 4096)              # the capacity of a batch scene


def scene(sb, cap, n_particles, pairs, layout=1, pmap=None, bmap=None, lengths=None):
    """n_particles particles on a grid of spacing 25 and one beam per pair (particle SLOT pairs); pmap / bmap: the data index of
    every slot (None: its own); lengths: the rest length per beam (None: 10)"""
    maxP, maxB = cap
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    pd = np.arange(n_particles) if pmap is None else np.asarray(pmap)
    bd = np.arange(len(pairs)) if bmap is None else np.asarray(bmap)
    buf = sb.Buffers(layout, maxP, maxB)
    buf.particles[pd, 0] = 20.0 + 25.0 * (np.arange(n_particles) % 32)
    buf.particles[pd, 1] = 20.0 + 25.0 * (np.arange(n_particles) // 32)
    rec = np.zeros(len(pairs), buf.beams.dtype)
    rec["a"], rec["b"] = pd[pairs[:, 0]], pd[pairs[:, 1]]
    rec["length"] = rec["target_length"] = rec["last_length"] = 10.0 if lengths is None else np.asarray(lengths, np.float32)
    rec["spring"], rec["damp"], rec["yield_strain"], rec["strain_break_limit"] = MAT
    buf.beams[bd] = rec
    buf.mapping[:n_particles] = pd
    buf.mapping[maxP:maxP + len(pairs)] = bd
    buf.particle_count, buf.beam_count = n_particles, len(pairs)
    return buf


def star(sb):
    """1024 particles / 4096 beams: particle 0 joined to each of the other 1023, the remaining 3073 beams parallel duplicates, the
    hub the record's high endpoint in every third beam, every beam its own rest length: a degree of 4096"""
    j = np.arange(CORNER_CAP[1])
    other = 1 + j % (CORNER_CAP[0] - 1)
    pairs = np.where((j % 3 == 0)[:, None], np.stack([other, 0 * j], 1), np.stack([0 * j, other], 1))
    return scene(sb, CORNER_CAP, CORNER_CAP[0], pairs, layout=2, lengths=10.0 + j % 97)


def corner_scenes(sb):
    """the capacity corners of one batch: the star, 2 particles / 1 beam, particles and no beam, never uploaded, a chain of 65
    particles whose runs of nbr cross a wave boundary"""
    return [star(sb), scene(sb, CORNER_CAP, 2, [(1, 0)], layout=2), scene(sb, CORNER_CAP, 7, [], layout=2), None,
            scene(sb, CORNER_CAP, 65, [(i, i + 1) for i in range(64)], layout=2)]
