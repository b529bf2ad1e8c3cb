"""What the GPU tests of the batch's queries share (tests/test_gpu_batch_raycast*.py, tests/test_gpu_batch_nearest*.py): a batch of
the case set's capacity, the call into outputs pre-filled with a pattern -- an unwritten word would show --, the comparison with
the restatement on what load_scene returns now, and every byte the other reports can see."""
import numpy as np

import batch_raycast_cases as cases
from batch_harness import load_all, make_batch, upload_each

OFF, GRID = 0, 2


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def batch(sb, bufs, mode=OFF, cap=cases.CAP, layout=cases.LAYOUT):
    be = make_batch(sb, dict(layout=layout, cap=cap, bufs=bufs, mode=mode), mode=mode)
    upload_each(be, bufs)
    return be


def raw(be):
    """every byte the other reports can see: state rows, summary, bodies"""
    p, b, a = be.state_tensors()
    return [x.cpu().numpy().tobytes() for x in (p, b, a, be.summary(), *be.bodies())]


def query(method, ref_of, result, same, outs):
    """(ask, check) of one query: BatchEngine.<method> against ref_of (the restatement of a batch) as the named tuple `result`,
    compared by `same`.  outs: (keyword, shape after [n_scenes, k] or None for the counts' [n_scenes, 4], torch dtype name) each."""
    def ask(be, rows, labels=None):
        """the outputs as numpy, written into tensors the test filled with a pattern first: every word is written"""
        import torch
        n, k = be.n_scenes, rows.shape[1]
        fill = lambda tail, dt: torch.full((n, 4) if tail is None else (n, k) + tail, -1515870811 if dt == "int32" else -7.25,   # 0xA5A5A5A5
                                           dtype=getattr(torch, dt), device="cuda")
        got = getattr(be, method)(dev(rows), labels=labels if labels is None or labels is True else dev(labels),
                                  **{name: fill(tail, dt) for name, tail, dt in outs})
        return result(*(x.cpu().numpy() for x in got))

    def check(be, bufs, rows, labels=None, what=""):
        """the call == the restatement on what load_scene returns now; returns (the scenes as read back, the result)"""
        now = load_all(be, bufs)
        want = ref_of(now, rows, labels=labels)
        got = ask(be, rows, labels)
        print(what, "counts", got.counts[:12].tolist(), "want", want.counts[:12].tolist())
        assert same(got, want) == [], what
        return now, got
    return ask, check
