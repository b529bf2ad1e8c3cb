'use strict';
// GPU test of the picture through the Node path: JS host -> N-API addon -> sb_render.  The PPM the worker / facade render()
// returns equals renderPPM (host/render.js) of the state loadBuffers() reads back, byte for byte (tests/test_gpu_render_node.py).
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const h = require('..');

const GOLDEN = path.resolve(__dirname, '..', '..', '..', 'tests', 'golden');
const rd = (f) => { const b = fs.readFileSync(path.join(GOLDEN, f)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); };
const out = { ok: false, cases: [] };

const same = (what, got, want) => {
    let diff = 0;
    if (got.length === want.length) for (let i = 0; i < got.length; i++) if (got[i] !== want[i]) diff++;
    assert.strictEqual(got.length, want.length, what + ': length');
    assert.strictEqual(diff, 0, what + ': ' + diff + ' bytes differ from renderPPM');
    out.cases.push({ what, bytes: got.length });
};

(async () => {
    // the default scene through the facade: 2 frames, then render() against renderPPM of the saved state
    const engine = new h.WGPUSoftbodyEngine(null, 0, { particleRadius: 10, subticks: 64 });
    assert.strictEqual(await engine.loadSnapshot(rd('default_scene_v1.snapshot')), true);
    await engine.run(2);
    const snap = await engine.saveSnapshot();
    const m = new h.BufferMapper(1 << 22, { layout: 1 });
    assert.strictEqual(m.loadSnapshotbuffer(snap), true);
    for (const res of [500, 512, 77]) same('default scene ' + res, await engine.render({ resolution: res }), h.renderPPM(m, { resolution: res }));
    same('default scene, default options', await engine.render(), h.renderPPM(m, {}));
    same('default scene, overrides', await engine.render({ resolution: 300, boundsSize: 812.5, particleRadius: 14.25 }),
        h.renderPPM(m, { resolution: 300, boundsSize: 812.5, particleRadius: 14.25 }));
    await engine.destroy();

    // the config-1 lattice through the worker: wide layout, tiled path, 1000 substeps + a frame (delete pass)
    const w = new h.WGPUSoftbodyEngineWorker(null, { layout: 2, maxParticles: 2048, maxBeams: 8192, boundsSize: 1500, collisionMode: h.COLLIDE.OFF,
        path: h.PATH.TILED, tileParticles: 256 });
    let ids = { particleId: 0, beamId: 0 };
    ids = h.addRectangle(w.bufferMapper, ids, 100, 100, 25, 32, 32, 50, 700, 0.2, 0.5, false);
    w.bufferMapper.writeState();
    await w.writeBuffers();
    await w.step(1000);
    await w.frame();
    const pic = await w.render({ resolution: 640 });
    await w.loadBuffers();
    same('config-1 lattice 640', pic, h.renderPPM(w.bufferMapper, { resolution: 640, boundsSize: 1500, particleRadius: 10 }));
    await w.destroy();
    out.ok = true;
    console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); console.log(JSON.stringify(out)); process.exit(1); });
