"""checkpoint() / restore() through the Node path (JS host -> N-API addon -> sb_checkpoint_device / sb_restore_device):
host/test/checkpoint.gpu.test.js rewinds a run through the worker and the facade and compares the read-backs byte for byte."""
import pytest

from test_node_host import needs_node, run_node


@needs_node
@pytest.mark.gpu
def test_checkpoint_restore_through_node():
    r = run_node("checkpoint.gpu.test.js")
    assert r["ok"] and r["restores"] == 2, r
