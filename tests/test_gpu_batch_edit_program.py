"""The editing calls of a BatchEngine run as a PROGRAM: about thirty batch-wide ops per seed (tests/batch_edit_cases.py) -- frame,
step, delete pass, cut, add_beams, reset, checkpoint, fork and dry runs -- on twelve scenes, against one host model per scene
(tests/batch_edit_model.py: the oracle, cut_ref and batch_add_beams_ref, nothing of a kernel).  The state the calls share is where
a long sequence can drift: slot-indexed pending flags, the beam mapping that delete passes compact, data indices that must be free
in the current and in the reset state, reset state that a fork replaces.  Every comparison is bit for bit.

What is compared of a scene.  load_scene writes the live particle rows and the record of every beam data index that an upload or
an add ever used, into the buffers it is given; the model reads into a copy of the same upload.  While a scene is still in the
lineage of that upload and no reset has undone an add (`exact` in the model), batch and model start from the same base copy and
WHOLE buffers are compared: both mappings with their stale entries behind the live counts, every particle row, every beam record.
After a reset that undid an add, the undone index exports the add's material beside the reset state's beam state -- a row no
live slot names, which load_scene's contract does not define -- so from then on the scene is compared at what the contract does
define: counts, metadata, the live part of both mappings, every particle row and beam record at a live data index.

The oracle runs all-pairs for both collision modes, as tests/test_gpu_batch_cut.py argues.  tests/test_batch_edit_model_cpu.py
shows on the CPU that the programs stay finite, reach the cases they are for, and catch three wrong models."""
import numpy as np
import pytest

import batch_bodies_ref
import batch_contacts_ref
import batch_edit_cases as cases
import batch_edit_model as model
import graph_ref
from batch_harness import upload_each

pytestmark = pytest.mark.gpu

ALLPAIRS, GRID = 1, 2
LC, SJ = 2, 4


def dev(a, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()


def apply_to_batch(be, op):
    """the op on the batch; returns the tensors the call returns, as numpy"""
    import torch
    k = op[0]
    if k == "frame":
        be.frame(op[1])
    elif k == "step":
        be.step(op[1])
    elif k == "delete":
        be.delete_pass()
    elif k == "cut":
        hit, counts = be.cut(dev(op[1]), dry_run=op[2], hit=True)
        return dict(hit=hit.cpu().numpy(), counts=counts.cpu().numpy())
    elif k == "add":
        res, counts = be.add_beams(dev(op[1]), length_current=bool(op[2] & LC), skip_joined=bool(op[2] & SJ), dry_run=op[3])
        return dict(result=res.cpu().numpy(), counts=counts.cpu().numpy())
    elif k in ("reset", "checkpoint"):
        getattr(be, k)(torch.from_numpy(op[1]).cuda())
    elif k == "fork":
        be.fork(dev(op[1]), as_reset=op[2])
    else:
        raise ValueError(op)
    return {}


def raw_state(be):
    return [x.cpu().numpy().tobytes() for x in be.state_tensors()]


def read_back(be, models):
    return [be.load_scene(i, m.template.copy()) if m.loaded else None for i, m in enumerate(models)]


@pytest.mark.parametrize("mode", [pytest.param(GRID, id="grid"), pytest.param(ALLPAIRS, id="walk")])
@pytest.mark.parametrize("seed", cases.SEEDS)
def test_edit_program(sb, seed, mode):
    bufs, ops = cases.program(sb, seed)
    models = cases.make_models(sb, bufs)
    # (grid_min_particles = 1: the cells run in every scene of the program)
    be = sb.BatchEngine(n_scenes=cases.N, layout=cases.LAYOUT, max_particles=cases.CAP[0], max_beams=cases.CAP[1], collision_mode=mode,
                        grid_min_particles=1 if mode == GRID else None)
    upload_each(be, bufs)
    for k, op in enumerate(ops):
        where = "seed %d, op %d (%s)" % (seed, k, model.kind(op))
        before = None if model.changes_state(op) else raw_state(be)
        got, want = apply_to_batch(be, op), model.apply(models, op)
        got["summary"], want["summary"] = be.summary().cpu().numpy()[:, [1, 2, 3]], model.summary_words(models)
        diff = model.outputs_difference(got, want)
        if diff is not None:
            bad = [i for i in range(cases.N) if np.asarray(got[diff])[i].tobytes() != np.asarray(want[diff]).astype(got[diff].dtype)[i].tobytes()]
            print(where, diff, "scenes", bad, "got", np.asarray(got[diff])[bad[0]].tolist(), "want", np.asarray(want[diff])[bad[0]].tolist())
        assert diff is None, "%s: `%s` differs" % (where, diff)
        if before is not None:
            assert raw_state(be) == before, where + ": a dry run changed the state"
        if model.changes_state(op) or k % 5 == 4 or k == len(ops) - 1:
            for i, (g, m) in enumerate(zip(read_back(be, models), models)):
                if m.loaded:
                    diff = model.scene_difference(g, m.current(), m.exact)
                    assert diff is None, "%s, scene %d: %s differs (whole buffers: %s)" % (where, i, diff, m.exact)
                else:
                    with pytest.raises(sb.engine.EngineError):
                        be.load_scene(i, bufs[0].copy())
    now = [m.current() if m.loaded else None for m in models]
    exact = [m.exact for m in models if m.loaded]
    assert len(exact) >= 6 and any(exact) and not all(exact), "both comparisons were made"
    g = graph_ref.Graph(*(x.cpu().numpy() for x in be.graph(ends=True, material=True, adjacency=True)))
    assert graph_ref.same(g, graph_ref.graph_of(now, *cases.CAP)) == []
    labels, counts = (x.cpu().numpy() for x in be.bodies())
    wl, _, wc = batch_bodies_ref.bodies_of(now, cases.CAP[0])
    assert np.array_equal(labels, wl) and np.array_equal(counts, wc)
    touch, ccounts = (x.cpu().numpy() for x in be.contacts())
    wt, _, wcc = batch_contacts_ref.contacts_of(now, cases.CAP[0])
    assert np.array_equal(touch, wt) and np.array_equal(ccounts, wcc)
    if mode == GRID:
        assert be.info("cell_substeps") > 0
    be.destroy()
