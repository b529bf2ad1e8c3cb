"""The batch's fuzz family (tests/batch_fuzz_cases.py) without a GPU: the oracle alone runs every seed and must stay finite in
every scene at every op; over the committed seeds the family must bite -- breaks removed where the break flags end in a partial
word, yield, pile-ups on the contact cells that cross the bucket's capacity within one launch, crossed tie-breaks, full capacities,
odd subticks, all six instances of the kernel; and the boundary capacities are the boundaries of the restated LDS formula."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
import batch_fuzz_cases as fz  # noqa: E402
import batch_grid_cases as gc  # noqa: E402

_survey = {}


def crowding(case, ref):
    """(most simultaneous contacts of a particle, fullest contact cell) at the oracle's present positions: what the next substep
    reads."""
    p = fz.live_particles(ref)[:, :2]
    g, cell = gc.cell_geometry(case["bounds"], case["radius"], case["cap"][0])
    d = p[None, :, :] - p[:, None, :]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype("f4"))
    contact = ((dist == 0) | (dist < np.float32(2.0 * case["radius"]))) & ~np.eye(len(p), dtype=bool)
    with np.errstate(invalid="ignore"):
        cx, cy = (np.clip(np.nan_to_num(np.floor(p[:, a] / cell), nan=0.0), 0, g - 1).astype(int) for a in (0, 1))
    return int(contact.sum(1).max()), int(np.bincount(cy * g + cx).max())


def survey(sb, oracle, seed):
    """The oracles of one case through its program, once per session.  Every scene is looked at after every op; the clump scene of a
    case whose clump takes the cells is stepped substep by substep (the same state: asserted against a second oracle stepped
    per op)."""
    if seed in _survey:
        return _survey[seed]
    case = fz.case(sb, seed)
    refs = [None if b is None else fz.make_oracle(oracle, case, b) for b in case["bufs"]]
    watch = case["clump"] if case["clump"] is not None and fz.takes_cells(case, case["clump"]) else None
    twin = fz.make_oracle(oracle, case, case["bufs"][watch]) if watch is not None else None
    out = dict(case=case, finite=True, first_bad=None, removed=False, yielded=False, contacts=0, crossed=False, launches=[])
    st = refs[case["empty"]].subticks
    assert st == (case["subticks"] + 1) // 2 * 2

    def launch(n):
        full = []
        for _ in range(n):
            c, f = crowding(case, twin)
            out["contacts"] = max(out["contacts"], c)
            full.append(f)
            twin.step(1)
        out["launches"].append((min(full), max(full)))
        out["crossed"] |= min(full) <= fz.CELL_K < max(full)

    for k, op in enumerate(case["program"]):
        before = [None if r is None else int(r.metadata[6]) for r in refs]
        bc.apply_to_oracles(refs, op)
        if twin is not None:
            if op[0] == "frame":
                for _ in range(op[1]):
                    launch(st)
                    twin.delete_pass()
            elif op[0] == "step":
                launch(op[1])
            else:
                bc.apply_to_oracles([None] * watch + [twin], op)
            a, b = refs[watch].load_buffers(case["bufs"][watch].copy()), twin.load_buffers(case["bufs"][watch].copy())
            assert np.array_equal(a.particles.view("u4"), b.particles.view("u4")) and np.array_equal(a.mapping, b.mapping)
        for i, r in enumerate(refs):
            if r is None:
                continue
            if not np.isfinite(fz.live_particles(r)).all() and out["finite"]:
                out["finite"], out["first_bad"] = False, "scene %d (%s) after op %d %s" % (i, case["kinds"][i], k, op[:2])
            B = int(r.metadata[6])
            out["removed"] |= B < before[i]
            live = r.beams[r.mapping[r.max_particles:r.max_particles + B].astype(np.int64)]
            out["yielded"] |= bool((live["target_length"] != live["length"]).any())
    assert all(int(r.metadata[1]) == 0 and int(r.metadata[6]) == 0 for r in [refs[case["empty"]]])
    _survey[seed] = out
    return out


@pytest.mark.parametrize("seed", range(fz.SEED0, fz.SEED0 + fz.COUNT))
def test_every_scene_of_the_seed_stays_finite(sb, oracle, seed):
    s = survey(sb, oracle, seed)
    assert s["finite"], "seed %d: %s" % (seed, s["first_bad"])


def test_a_case_is_what_the_issue_asks_for(sb):
    for seed in range(fz.NSEEDS):
        c = fz.case(sb, seed)
        st = (c["subticks"] + 1) // 2 * 2
        live = [b for b in c["bufs"] if b is not None]
        assert 8 <= len(c["bufs"]) <= 12 and 6 <= len(c["program"]) <= 10
        assert gc.substeps_of(c["program"], st) <= 4 * st
        assert sum(b.particle_count > 256 for b in live) <= 2
        assert c["bufs"][c["never"]] is None and c["bufs"][c["empty"]].particle_count == 0
        assert c["bufs"][c["full_p"]].particle_count == c["cap"][0] and c["bufs"][c["full_b"]].beam_count == c["cap"][1]
        assert all((b.max_particles, b.max_beams, b.layout) == (*c["cap"], c["layout"]) for b in live)
        assert any(op[0] == "frame" for op in c["program"])
        assert c["bounds"] in fz.BOUNDS and c["radius"] in fz.RADII and c["subticks"] in fz.SUBTICKS
        if c["mode"] == fz.GRID:
            g, cell = gc.cell_geometry(c["bounds"], c["radius"], c["cap"][0])
            p = c["bufs"][c["clump"]]
            xy = p.particles[p.mapping[:p.particle_count].astype(np.int64), :2]
            cx, cy = (np.clip(np.floor(xy[:, a] / cell), 0, g - 1).astype(int) for a in (0, 1))
            assert np.bincount(cy * g + cx).max() >= 5
    assert fz.case(sb, 0) is fz.case(sb, 0)                      # drawn once, shared, never changed


def test_the_family_bites(sb, oracle):
    """Over the COMMITTED seeds, whatever SB_FUZZ_OFFSET says."""
    all_ = [survey(sb, oracle, seed) for seed in range(fz.NSEEDS)]
    cases = [s["case"] for s in all_]
    ragged = [s for s in all_ if s["case"]["cap"][1] % 32 != 0]
    assert sum(s["removed"] for s in ragged) >= 3, [s["case"]["seed"] for s in ragged if s["removed"]]
    assert any(s["yielded"] for s in all_)
    assert sum(s["contacts"] >= 5 for s in all_) >= 3, [s["contacts"] for s in all_]
    assert sum(s["crossed"] for s in all_) >= 3, [s["launches"] for s in all_ if s["launches"]]
    crossed_pairs = 0
    for c in cases:
        if c["coincident"] is None:
            continue
        buf = c["bufs"][c["coincident"]]
        slots = np.argsort(buf.mapping[:buf.particle_count].astype(np.int64))       # slot of each live data index, in data order
        data = np.sort(buf.mapping[:buf.particle_count].astype(np.int64))
        xy = buf.particles[data, :2]
        same = [(i, j) for i in range(len(xy)) for j in range(i + 1, len(xy)) if (xy[i] == xy[j]).all()]
        assert same, c["seed"]
        crossed_pairs += sum(slots[i] > slots[j] for i, j in same)                  # data i < data j, slot i > slot j
    assert crossed_pairs >= 1
    assert any(c["bufs"][c["full_p"]].particle_count == c["cap"][0] for c in cases)
    assert {48, 100, 63} <= {c["subticks"] for c in cases}
    assert {c["expect_variant"] for c in cases} == set(fz.VARIANTS)
    assert {c["cap"] for c in cases} >= {r for r in fz.TABLE if not isinstance(r[1], tuple)}


def test_boundary_capacities_are_the_boundaries_of_the_restated_formula(sb):
    seen = set()
    for seed in range(fz.NSEEDS):
        c = fz.case(sb, seed)
        row = fz.TABLE[seed % len(fz.TABLE)]
        if not isinstance(row[1], tuple):
            continue
        _, delta, with_cells = row[1]
        e = c["expect"]
        cell_bytes = fz.up16(fz.batch_cell_lds_bytes(e["cells_per_side"])) if e["collide"] == fz.CELLS else 0
        assert (e["collide"] == fz.CELLS) == with_cells and (cell_bytes > 0) == with_cells
        last = c["cap"][1] - delta
        assert fz.mats_fit(c["cap"][0], last, cell_bytes) and not fz.mats_fit(c["cap"][0], last + 1, cell_bytes)
        assert e["materials_in_lds"] == (delta == 0)
        assert e["lds_bytes"] <= fz.LDS_LIMIT and e["threads"] == 1024
        seen.add((delta, with_cells))
    assert seen == {(0, False), (1, False), (0, True), (1, True)}
    # the restatement against figures DESIGN.md 5.10 gives: 128 / 320 walks on 18.5 KB, 22.0 KB with 17 cells a side
    assert fz.batch_lds_bytes(128, 320, True) == 18528 and fz.batch_threads(128, 320) == 128
    assert fz.batch_lds_bytes(128, 320, True) + fz.up16(fz.batch_cell_lds_bytes(17)) == 22016
    assert fz.batch_threads(63, 700) == 192 and fz.batch_threads(64, 256) == 64 and fz.batch_threads(1024, 4096) == 1024
