"""The nine editing calls of a BatchEngine run as a PROGRAM: tests/test_gpu_batch_edit_program.py with add_particles mixed in
(tests/batch_spawn_model.py: about thirty batch-wide ops per seed on twelve scenes, against one host model per scene).  What a long
sequence can drift in here: the particle count and the reset particle count through reset, checkpoint, fork and masks, the "holds a
particle" bytes that a reset must clear, welds onto particles a reset removes.  Every comparison is bit for bit; what is compared of
a scene is what the edit-program test compares (whole buffers while the model calls the scene `exact`, else what load_scene's
contract defines), plus summary()'s particle count.  tests/test_batch_spawn_model_cpu.py shows on the CPU that the programs reach the
cases they are for and catch two wrong models."""
import numpy as np
import pytest

import batch_bodies_ref
import batch_contacts_ref
import batch_edit_model as model
import batch_spawn_model as spawn
import test_gpu_batch_edit_program as edit_program
from batch_harness import upload_each

pytestmark = pytest.mark.gpu

ALLPAIRS, GRID = 1, 2
SKIP_TOUCHING = 2


def apply_to_batch(be, op):
    if op[0] == "spawn":
        res, counts = be.add_particles(edit_program.dev(op[1]), skip_touching=bool(op[2] & SKIP_TOUCHING), dry_run=op[3])
        return dict(result=res.cpu().numpy(), counts=counts.cpu().numpy())
    return edit_program.apply_to_batch(be, op)


@pytest.mark.parametrize("mode", [pytest.param(GRID, id="grid"), pytest.param(ALLPAIRS, id="walk")])
@pytest.mark.parametrize("seed", spawn.SEEDS)
def test_spawn_program(sb, seed, mode):
    bufs, ops = spawn.program(sb, seed)
    models = spawn.make_models(sb, bufs)
    be = sb.BatchEngine(n_scenes=spawn.N, layout=spawn.LAYOUT, max_particles=spawn.CAP[0], max_beams=spawn.CAP[1], collision_mode=mode,
                        grid_min_particles=1 if mode == GRID else None)
    upload_each(be, bufs)
    for k, op in enumerate(ops):
        where = "seed %d, op %d (%s)" % (seed, k, spawn.kind(op))
        before = None if spawn.changes_state(op) else edit_program.raw_state(be)
        got, want = apply_to_batch(be, op), spawn.apply(models, op)
        got["summary"], want["summary"] = be.summary().cpu().numpy()[:, [0, 1, 2, 3]], spawn.summary_words(models)
        diff = model.outputs_difference(got, want)
        if diff is not None:
            bad = [i for i in range(spawn.N) if np.asarray(got[diff])[i].tobytes() != np.asarray(want[diff]).astype(got[diff].dtype)[i].tobytes()]
            print(where, diff, "scenes", bad, "got", np.asarray(got[diff])[bad[0]].tolist(), "want", np.asarray(want[diff])[bad[0]].tolist())
        assert diff is None, "%s: `%s` differs" % (where, diff)
        if before is not None:
            assert edit_program.raw_state(be) == before, where + ": a dry run changed the state"
        if spawn.changes_state(op) or k % 5 == 4 or k == len(ops) - 1:
            for i, (g, m) in enumerate(zip(edit_program.read_back(be, models), models)):
                if m.loaded:
                    diff = model.scene_difference(g, m.current(), m.exact)
                    assert diff is None, "%s, scene %d: %s differs (whole buffers: %s)" % (where, i, diff, m.exact)
                else:
                    with pytest.raises(sb.engine.EngineError):
                        be.load_scene(i, bufs[0].copy())
    now = [m.current() if m.loaded else None for m in models]
    labels, counts = (x.cpu().numpy() for x in be.bodies())
    wl, _, wc = batch_bodies_ref.bodies_of(now, spawn.CAP[0])
    assert np.array_equal(labels, wl) and np.array_equal(counts, wc)
    touch, ccounts = (x.cpu().numpy() for x in be.contacts())
    wt, _, wcc = batch_contacts_ref.contacts_of(now, spawn.CAP[0])
    assert np.array_equal(touch, wt) and np.array_equal(ccounts, wcc)
    held = np.stack([m.pex if m.loaded else np.zeros(spawn.CAP[0], bool) for m in models])
    assert np.array_equal(np.isnan(be.state_tensors()[0].cpu().numpy()[:, :, 0]), ~held), "the rows exported are the held ones"
    be.destroy()
