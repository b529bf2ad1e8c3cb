"""The picture through the Node host: worker / facade render() -> N-API -> sb_render equals host/render.js renderPPM of the
read-back state, byte for byte (host/test/render.gpu.test.js)."""
import pytest

from test_node_host import needs_node, run_node


@needs_node
@pytest.mark.gpu
def test_js_render_equals_render_ppm():
    r = run_node("render.gpu.test.js")
    assert r["ok"] and len(r["cases"]) == 6, r
