"""Engine.write_beams_device (sb_write_beams_device): target_length / last_length of every beam from rows in device
memory, into every copy the engine keeps of the beam -- equal to the same edit made on the host and uploaded, against the oracle; the
field mask; the round trip of what was just exported; the caller's renumbered slots after an upload that cut beams; the blocked
path's plastic promise; torch's stream ordered against the engine's.  All comparisons are bit for bit."""
import numpy as np
import pytest

from test_gpu_parity import ATOMIC, GRID, OFF, TILED, assert_same
from test_gpu_reupload import breaking_lattice, moved, without
from test_gpu_state_io import SCHEDULES, assert_same_run, check_export, corner_block, final, quiet_lattice

pytestmark = pytest.mark.gpu

NAN, NAN_PAYLOAD, NEG_ZERO = 0x7FC00000, 0x7FC12345, 0x80000000
_oracle_runs = {}


def engine(sb, buf, bounds, **kw):
    eng = sb.Engine(bounds_size=bounds, layout=buf.layout, max_particles=buf.max_particles, max_beams=buf.max_beams, **kw)
    eng.write_buffers(buf)
    return eng


def beam_rows(state):
    """data indices of the beams of `state`, in slot order"""
    return state.mapping[state.max_particles:state.max_particles + state.beam_count].astype(np.int64)


def beams_inside(state, particles):
    """data indices of the beams with both endpoints among the particle data indices `particles`"""
    rows = beam_rows(state)
    inside = np.zeros(state.max_particles, bool)
    inside[particles] = True
    return rows[inside[state.beams["a"][rows]] & inside[state.beams["b"][rows]]]


def far_block(upload, d, n=10):
    """the n x n lattice corner with the largest x and y (test_gpu_state_io.corner_block is the one with the smallest)"""
    P = upload.particle_count
    rows = upload.mapping[:P].astype(np.int64)
    xy = upload.particles[rows, :2].astype(np.float64)
    hi = xy.max(axis=0)
    sel = (xy[:, 0] > hi[0] - (n - 0.5) * d) & (xy[:, 1] > hi[1] - (n - 0.5) * d)
    assert sel.sum() == n * n
    return rows[sel]


def the_edit(upload, base):
    """(edited buffers, rows whose target changed, rows whose last changed): targets of a corner block's beams to 0.8 of their rest
    length, last lengths of the opposite block's beams to 1.1 of their value; one beam each with a NaN target, a -0.0 last length
    and a NaN with a payload as last length."""
    edited = base.copy()
    t_rows = beams_inside(base, corner_block(upload, 30.0))
    l_rows = beams_inside(base, far_block(upload, 30.0))
    assert t_rows.size >= 180 and l_rows.size >= 180 and not np.intersect1d(t_rows, l_rows).size
    edited.beams["target_length"][t_rows] = edited.beams["length"][t_rows] * np.float32(0.8)
    edited.beams["last_length"][l_rows] = edited.beams["last_length"][l_rows] * np.float32(1.1)
    rest = np.setdiff1d(beam_rows(base), np.concatenate([t_rows, l_rows]))
    special = rest[[rest.size // 3, rest.size // 2, 2 * rest.size // 3]]
    edited.beams["target_length"].view("<u4")[special[0]] = NAN
    edited.beams["last_length"].view("<u4")[special[1]] = NEG_ZERO
    edited.beams["last_length"].view("<u4")[special[2]] = NAN_PAYLOAD
    return edited, np.concatenate([t_rows, special[:1]]), np.concatenate([l_rows, special[1:]])


def device_rows(eng, edited):
    """the four state floats of `edited`'s beam records as the tensor write_beams_device takes (rows at data indices)"""
    import torch
    b = edited.beams
    rows = np.stack([b["target_length"], b["last_length"], b["strain"], b["stress"]], axis=1).astype("<f4")
    return torch.from_numpy(rows.view("<i4").copy()).to(torch.device("cuda", eng.device)).view(torch.float32)


def oracle_after(oracle, edited, bounds, mode, frames):
    key = (mode, frames, edited.particles.tobytes(), edited.beams.tobytes())
    if key not in _oracle_runs:
        ref = oracle.OracleEngine(bounds, 10.0, 64, edited.layout, mode, threads=16)
        ref.write_buffers(edited)
        for _ in range(frames):
            ref.frame()
        _oracle_runs[key] = ref.load_buffers(edited.copy())
    return _oracle_runs[key]


@pytest.mark.parametrize("what,mode,path,kw", [("blocked, collisions off", OFF, TILED, {}),
                                               ("tiled grid, 256-particle tiles", GRID, TILED, {"tile_particles": 256}),
                                               ("atomic", GRID, ATOMIC, {}), ("default, hybrid", GRID, 0, {})],
                         ids=["blocked", "tiled-grid", "atomic", "hybrid"])
def test_import_equals_host_edit(sb, oracle, what, mode, path, kw):
    """1: an edit imported through write_beams_device (A) == the same buffers uploaded (B) == the oracle given them, two frames
    later, bit for bit.  What each case is there for: the tiled-grid case cuts many beams (every COPY of a beam must be written,
    asserted through "beam_copies"); the blocked case needs the second target half and the plastic flag (a tile that is not flagged
    never reads its targets).  Which of these writes which test notices, and on which half of the double buffers, is worked out
    over a model of the store in tests/test_state_io_model_cpu.py; tests/test_gpu_state_io_halves.py runs the import on each half."""
    buf = quiet_lattice(sb)
    A = engine(sb, buf, 6000.0, collision_mode=mode, path=path, **kw)
    for _ in range(3):
        A.frame()
    base = A.load_buffers(buf.copy())
    if what.startswith("tiled"):
        assert A.info("beam_copies") > base.beam_count * 1.05, "the tiling must cut many beams"
    if what.startswith("default"):
        assert A.info("hybrid_launches") > 0, "blocked launches must have run before the import"
    edited, t_rows, l_rows = the_edit(buf, base)
    A.write_beams_device(device_rows(A, edited), target_length=True, last_length=True)
    imported = A.load_buffers(base.copy())      # the import, read back before any step
    assert imported.beams.tobytes() == edited.beams.tobytes(), what + ": the import is not the edit"
    assert imported.particles.tobytes() == base.particles.tobytes() and A.info("substeps_done") == 3 * 64
    B = engine(sb, edited, 6000.0, collision_mode=mode, path=path, **kw)
    for e in (A, B):
        e.frame()
        e.frame()
    got_a, got_b = A.load_buffers(edited.copy()), B.load_buffers(edited.copy())
    if what.startswith("default"):
        assert A.info("hybrid_launches") > 0
    A.destroy()
    B.destroy()
    assert_same(got_a, got_b, what + ": import vs host edit")
    assert_same(got_a, oracle_after(oracle, edited, 6000.0, mode, 2), what + ": import vs oracle")
    assert not np.array_equal(got_a.particles[corner_block(buf, 30.0)], base.particles[corner_block(buf, 30.0)])


@pytest.mark.parametrize("what,mode,path,kw", [SCHEDULES[3], SCHEDULES[4], SCHEDULES[0]], ids=["blocked", "tiled-grid", "atomic"])
def test_field_mask(sb, what, mode, path, kw):
    """2: target_length only leaves last_length as it was, and vice versa; seen through the export and sb_load_buffers."""
    buf = breaking_lattice(sb)
    eng = engine(sb, buf, 4000.0, collision_mode=mode, path=path, **kw)
    eng.frame()
    eng.step(5)
    base = eng.load_buffers(buf.copy())
    rows = beam_rows(buf)
    edited = base.copy()
    edited.beams["target_length"][rows] = base.beams["target_length"][rows] * np.float32(1.01)
    edited.beams["last_length"][rows] = base.beams["last_length"][rows] * np.float32(0.99)
    edited.beams["target_length"].view("<u4")[rows[5]] = NAN_PAYLOAD
    edited.beams["last_length"].view("<u4")[rows[6]] = NAN_PAYLOAD
    edited.beams["strain"][rows] = 123.0    # never imported
    edited.beams["stress"][rows] = -7.0
    t = device_rows(eng, edited)
    for target, last in ((True, False), (False, True)):
        eng.write_beams_device(t, target_length=target, last_length=last)
        state = check_export(eng, buf, "%s: fields %s" % (what, (target, last)))
        exp = base.copy() if target else edited.copy()     # the second round sits on top of the first
        exp.beams["strain"], exp.beams["stress"] = base.beams["strain"], base.beams["stress"]
        if target:
            exp.beams["target_length"] = edited.beams["target_length"]
        assert state.beams.tobytes() == exp.beams.tobytes(), "%s: fields %s" % (what, (target, last))
        prow = buf.mapping[:buf.particle_count].astype(np.int64)
        assert state.particles[prow].tobytes() == base.particles[prow].tobytes() and state.beam_count == base.beam_count
    eng.destroy()


@pytest.mark.parametrize("lay,what,mode,path,kw", [pytest.param(lay, *s, id="%s-v%d" % (s[0], lay)) for s in SCHEDULES for lay in (1, 2)])
def test_round_trip(sb, lay, what, mode, path, kw):
    """3: importing the beam rows just exported, at a frame boundary and mid-frame with flags pending, changes nothing."""
    buf = breaking_lattice(sb, layout=lay)
    kw = dict(collision_mode=mode, path=path, **kw)
    N, I = engine(sb, buf, 4000.0, **kw), engine(sb, buf, 4000.0, **kw)

    def trip():
        t = I.state_tensors()
        I.write_beams_device(t["beams"], True, True)

    for f in range(3):
        for e in (N, I):
            e.frame()
        if f == 1:
            trip()
    for e in (N, I):
        e.step(5)
    trip()
    for _ in range(3):
        for e in (N, I):
            e.frame()
    out = final(I, buf), final(N, buf)
    N.destroy()
    I.destroy()
    assert out[1][1][1] < buf.beam_count, "beams must have broken"
    assert_same_run(out[0], out[1], what + ": importing what was exported changed the run")


@pytest.mark.parametrize("what,mode,path,kw", [SCHEDULES[3], SCHEDULES[4], SCHEDULES[0]], ids=["blocked", "tiled-grid", "atomic"])
def test_after_a_cutting_upload(sb, what, mode, path, kw):
    """4: the caller's slots are renumbered by an upload that cut beams (records at shuffled data indices): the rows at the NEW data
    indices are the ones read, and the rows of beams that are gone are inert.  == the same edit uploaded."""
    first = breaking_lattice(sb)
    cut = without(moved(first, 8), np.random.default_rng(11).random(first.beam_count) >= 0.01, shuffle_mapping=5)
    A = engine(sb, first, 4000.0, collision_mode=mode, path=path, **kw)
    A.frame()
    A.write_buffers(cut)
    assert A.info("uploads_edited") == 1
    edited = cut.copy()
    rows = beam_rows(cut)
    edited.beams["target_length"][rows] = cut.beams["target_length"][rows] * np.float32(0.97)
    edited.beams["last_length"][rows] = cut.beams["last_length"][rows] * np.float32(1.02)
    t = device_rows(A, edited)
    unused = np.setdiff1d(np.arange(cut.max_beams), rows)
    if unused.size:                               # rows of no beam of the latest upload: never read
        import torch
        t[torch.from_numpy(unused).to(t.device), :2] = 1.0e9
    A.write_beams_device(t, True, True)
    state = check_export(A, cut, what + ": after the import")
    assert state.beams[rows].tobytes() == edited.beams[rows].tobytes()
    B = engine(sb, first, 4000.0, collision_mode=mode, path=path, **kw)
    B.frame()
    B.write_buffers(edited)
    for e in (A, B):
        e.frame()
        e.frame()
        e.step(5)
    out = final(A, edited), final(B, edited)
    A.destroy()
    B.destroy()
    assert_same_run(out[0], out[1], what + ": import vs upload of the cut scene")


def test_plastic_promise(sb):
    """5: blocked path.  Targets equal to the rest lengths into a pristine scene: no tile's plastic flag is raised; one differing
    target: at least one; the run then equals the host-edit run."""
    buf = quiet_lattice(sb)
    A = engine(sb, buf, 6000.0, collision_mode=OFF, path=TILED)
    assert A.info("substeps_per_launch") > 1 and A.info("plastic_tiles") == 0
    base = A.load_buffers(buf.copy())
    rows = beam_rows(buf)
    same = base.copy()
    same.beams["target_length"][rows] = base.beams["length"][rows]
    A.write_beams_device(device_rows(A, same))
    assert A.info("plastic_tiles") == 0, "an import of the rest lengths raised a plastic flag"
    edited = base.copy()
    edited.beams["target_length"].view("<u4")[rows[rows.size // 2]] += 1      # one bit
    A.write_beams_device(device_rows(A, edited))
    assert A.info("plastic_tiles") >= 1
    B = engine(sb, edited, 6000.0, collision_mode=OFF, path=TILED)
    for e in (A, B):
        e.frame()
        e.step(5)
    got_a, got_b = A.load_buffers(edited.copy()), B.load_buffers(edited.copy())
    A.destroy()
    B.destroy()
    assert_same(got_a, got_b, "one differing target: import vs host edit")


def test_torch_ordering(sb):
    """6: a tensor produced on torch's stream right before the call, no explicit sync == the same edit through the host."""
    buf = breaking_lattice(sb)
    out, tpl = [], None
    for device_side in (False, True):
        eng = engine(sb, buf, 4000.0, collision_mode=GRID)
        eng.frame()
        if device_side:
            t = eng.state_tensors()
            rows = t["beams"] * 1.0
            rows[t["beam_alive"].bool(), 0] *= 0.95     # (a removed beam's row would be written too: the host edit cannot reach it)
            eng.write_beams_device(rows)
        else:
            tpl = eng.load_buffers(buf.copy())
            h = tpl.copy()
            h.beams["target_length"] *= np.float32(0.95)
            eng.write_buffers(h)
        eng.frame()
        out.append(eng.load_buffers(tpl.copy()))
        eng.destroy()
    assert_same(out[1], out[0], "torch edit vs host edit")
