"""Scenes and label sets of the tests of Engine.body_summary() (sb_body_summary_device), shared by
tests/test_body_summary_cpu.py (the reference alone: what every scene must show) and tests/test_gpu_body_summary.py.

The block sizes the scenes are cut for are the kernels': SORT_KEYS keys to a block of the radix sort (which sorts Wn member keys
and, with their number read on the device, the groups), SCAN_WORDS words to a block of the scans; the scan of the block sums
itself takes SCAN_SUMS_BLOCK sums an iteration.  The head flags are Wn words, so that scan takes a second iteration from Wn = 2^19
on; the digit counts of a sort are 256 words per SORT_KEYS keys, Wn / 4096 blocks, so theirs starts at Wn = 2^21.
PAST holds a scene for each."""
import numpy as np

import batch_bodies_ref as br
import bodies_cases as bc
import summary_cases as sc
from batch_bodies_cases import path_edges

SORT_KEYS = 1024        # SBY_SORT
SCAN_WORDS = 1024       # SBQ_SCAN (sb_report.h)
SCAN_SUMS_BLOCK = 256   # SBQ_BLOCK
INT32_MIN = -2 ** 31


def with_velocities(buf, seed):
    """every particle a velocity of its own, magnitudes spread over forty binary orders (summary_cases.case_cut's): the double
    sums round, so the order of the additions shows"""
    rng = np.random.default_rng(seed)
    idx = buf.mapping[:buf.particle_count].astype(np.int64)
    n = len(idx)
    buf.particles[idx, 2:4] = ((rng.standard_normal((n, 2)) * 3.0 + (0.7, -1.3)) * np.exp2(-rng.integers(0, 40, (n, 2)))).astype("f4")
    return buf


def graph(sb, cap, n, edges, seed, **kw):
    buf, D = bc.graph_scene(sb, cap, n, edges, seed, **kw)
    return with_velocities(buf, seed + 100)


def singles(sb, n, cap=None, seed=21):
    """n free particles, each a group of its own under bodies' labels: n keys for the group sort"""
    return graph(sb, cap or (n + 7, 4), n, [], seed)


SMALL = {
    "path 8 in 8/8": lambda sb: graph(sb, (8, 8), 8, path_edges(8), 31),
    "two pairs in 65/64": lambda sb: graph(sb, (65, 64), 4, [(0, 1), (2, 3)], 32),
    "path 65 in 65/64": lambda sb: graph(sb, (65, 64), 65, path_edges(65), 33),
    "two particles": lambda sb: graph(sb, (2, 4), 2, [(0, 1)], 34),
    "no particles": lambda sb: sb.Buffers(2, 16, 16),
}

BIG = {
    "path 4097": lambda sb: graph(sb, (5000, 5000), 4097, path_edges(4097), 2),
    "16 pieces of 256": lambda sb: graph(sb, (4096, 4096), 4096, path_edges(4096, 256), 4),
    "512 pairs": lambda sb: graph(sb, (1024, 1024), 1024, [(2 * k, 2 * k + 1) for k in range(512)], 5),
    "star 1024": lambda sb: graph(sb, (1100, 1100), 1024, [(1023, k) for k in range(1023)], 7, top=1023),
    "shuffled 65536, many bodies": lambda sb: graph(sb, (bc.N, bc.N), bc.N, path_edges(bc.N, 3), 8),
}

# groups one less than, exactly, and one more than the keys of a sort block (= the words of a scan block)
EDGES = {"%d singles" % n: (lambda sb, n=n: singles(sb, n)) for n in (SORT_KEYS - 1, SORT_KEYS, SORT_KEYS + 1)}

PAIRED = 1024           # particle numbers of "2^18 + 1025 particles" that are joined in pairs
N_PAST = (1 << 18) + 1025


def position_count(buf):
    """Wn: the smallest power of two at least the highest data index in use + 1 (what a call sorts and scans over)"""
    return sc.sr.pow2_at_least(int(buf.mapping[:buf.particle_count].max()) + 1) if buf.particle_count else 1


def scan_blocks(wn):
    """(blocks of the scan of a sort's digit counts, blocks of the scan of the head flags) at Wn positions"""
    return 256 * ((wn + SORT_KEYS - 1) // SORT_KEYS) // SCAN_WORDS, (wn + SCAN_WORDS - 1) // SCAN_WORDS


# past 256 scan blocks (SCAN_SUMS_BLOCK): the second iteration of the scan of the block sums, with its carry
PAST = {
    # 17 bodies over 1.5 M data indices: Wn = 2^21, 512 blocks in the scan of the digit counts (and 2048 in the flag scan)
    "sparse up to index 2^20+": lambda sb: graph(sb, (3 << 19, 5000), 4097, path_edges(4097, 256), 41),
    # the same graph where the capacity, a caller's word of "no group", takes 22 bits: 8-bit digits in the member sort
    "sparse in capacity 2^21 + 1": lambda sb: graph(sb, ((1 << 21) + 1, 5000), 4097, path_edges(4097, 256), 43),
    # 512 pairs and 2^18 + 1 single particles: Wn = 2^19, 512 blocks in the flag scan, 262 657 groups for the rank sort
    "2^18 + 1025 particles, pairs and singles": lambda sb: graph(sb, (N_PAST + 1023, 2048), N_PAST, [(2 * k, 2 * k + 1) for k in range(PAIRED // 2)], 42),
}

_cache = {}
_labels = {}


def scene(sb, name):
    """built once per process; not to be written to"""
    if name not in _cache:
        table = SMALL if name in SMALL else BIG if name in BIG else EDGES if name in EDGES else PAST
        _cache[name] = table[name](sb)
    return _cache[name]


def body_labels(buf):
    """bodies_ref's labels; of a scene of PAST (never written to) once per process"""
    for name in PAST:
        if _cache.get(name) is buf:
            if name not in _labels:
                _labels[name] = br.bodies_ref(buf)[0]
                _labels[name].setflags(write=False)
            return _labels[name]
    return br.bodies_ref(buf)[0]


def sparse_in_big_capacity(sb, cap=1 << 20):
    """(wide, tight): a 32 x 31 lattice (992 particles) permuted behind an offset in capacity 2^20 -- the tables end near data
    index 1050, so ten of twenty levels run -- and the same records at capacity 1100 (W = 2048)"""
    lat = with_velocities(sb.scenes.lattice_buffers(32, 31, d=30.0, origin=(100.0, 100.0), strain_limit=0.5, layout=2), 9)
    nb = lat.beam_count
    return sc.permuted(sb, lat, cap, nb + 200, 50, 100), sc.permuted(sb, lat, 1100, nb + 200, 50, 100)


def caller_labels(buf, which):
    """label sets of the caller's own at data indices"""
    maxP = buf.max_particles
    d = np.arange(maxP, dtype=np.int64)
    if which == "stripes":          # five interleaved groups, labels far apart
        lab = (d % 5) * (maxP // 5)
    elif which == "outside":        # -1, max_particles and INT32_MIN put a particle into no group; the rest is one group
        lab = np.full(maxP, maxP - 1, np.int64)
        lab[d % 4 == 0], lab[d % 4 == 1], lab[d % 7 == 3] = -1, maxP, INT32_MIN
    elif which == "split":          # a connected body split into halves by data index: the beams between them belong to nobody
        lab = np.where(d < maxP // 2, 3, 0)
    elif which == "uneven":         # groups of 200, 300 and the rest of the particles, by slot: sizes whose low bytes lie on both sides of 128
        lab = np.full(maxP, -1, np.int64)
        idx = buf.mapping[:buf.particle_count].astype(np.int64)
        lab[idx[:200]], lab[idx[200:500]], lab[idx[500:]] = 7, 9, 11
    elif which == "bodies, some outside":   # bodies' own labels, but every 384th data index in no group (-1, max_particles, INT32_MIN)
        lab = body_labels(buf).astype(np.int64)
        lab[d % 1152 == 5], lab[d % 1152 == 389], lab[d % 1152 == 773] = -1, maxP, INT32_MIN
    else:
        raise ValueError(which)
    return lab.astype(np.int32)


# ---- the call's own order on the CPU, for the tests that show what a scene reaches (tests/test_body_summary_cpu.py)
def bits_for(most):
    """sby_bits: the bits that hold every value 0 .. most"""
    return max(1, int(most).bit_length())


def digit_plan(bits):
    """[(shift, width)] of the passes of a sort by `bits` key bits: digits of equal width, at most 8 bits"""
    passes = (bits + 7) // 8
    per = (bits + passes - 1) // passes
    return [(at, min(per, bits - at)) for at in range(0, bits, per)]


def sorted_positions(buf, labels, own):
    """(g [Wn], d [Wn], none): the group word and the data index at every sorted position of a call -- members by group, then by
    the bit-reversed data index; what is in no group behind them under the word `none` (own: the engine's bodies, whose `none` is
    the highest data index in use + 1; else the capacity)"""
    import body_summary_ref as yr
    wn = position_count(buf)
    logw = wn.bit_length() - 1
    t = np.arange(wn, dtype=np.int64)
    d = np.zeros(wn, np.int64)
    for k in range(logw):
        d |= ((t >> k) & 1) << (logw - 1 - k)
    none = int(buf.mapping[:buf.particle_count].max()) + 1 if own else buf.max_particles
    grp = yr.groups_of(buf, labels)
    inside = d < buf.max_particles
    g = np.full(wn, none, np.int64)
    g[inside] = np.where(grp[d[inside]] >= 0, grp[d[inside]], none)
    order = np.argsort(g, kind="stable")
    return g[order], d[order], none


def hist_words(keys, n_max, bits, which):
    """The words k_bsum_hist leaves for pass `which` of a sort of `keys` (in the order the pass finds them: stably sorted by the
    digits below) out of n_max positions: digit-major, a count per sort block"""
    shift, width = digit_plan(bits)[which]
    keys = np.asarray(keys, np.int64)
    keys = keys[np.argsort(keys & ((1 << shift) - 1), kind="stable")]
    nb = (n_max + SORT_KEYS - 1) // SORT_KEYS
    dig = (keys >> shift) & ((1 << width) - 1)
    return np.bincount(dig * nb + np.arange(len(keys)) // SORT_KEYS, minlength=256 * nb)
