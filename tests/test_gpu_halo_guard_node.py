"""The halo guard through the Node host: partitionScene guard data, PeerExchanger(..., {guard: true}) throwing
RepartitionDueError, the addon's haloGuard / haloGuardStatus (host/test/halo_guard.gpu.test.js)."""
import pytest

from test_node_host import needs_node, run_node


@needs_node
@pytest.mark.gpu
def test_js_peer_exchanger_guard_throws_repartition_due():
    r = run_node("halo_guard.gpu.test.js")
    assert r["ok"] and r["fired"]["kinds"] and r["quietRefreshes"] == 9 * 64, r
