'use strict';
// GPU test of the connected bodies through the Node path: JS host -> N-API addon -> sb_bodies.  The labels and the counts the
// worker / facade bodies() return for the default scene after one frame are printed; tests/test_gpu_bodies.py compares them with
// what Python's Engine.bodies_host() gives for the same scene and capacity.
const assert = require('assert');
const h = require('..');

const out = { ok: false };

(async () => {
    const w = new h.WGPUSoftbodyEngineWorker(null, { layout: 1, maxParticles: 128, maxBeams: 320, boundsSize: 1000, particleRadius: 10,
        subticks: 64, collisionMode: h.COLLIDE.OFF });
    h.defaultScene(w.bufferMapper);
    w.bufferMapper.writeState();
    await assert.rejects(w.bodies(), /before writeBuffers/);
    await w.writeBuffers();
    await w.frame();
    const b = await w.bodies();
    assert.ok(b.labels instanceof Int32Array && b.labels.length === 128);
    assert.ok(Array.isArray(b.counts) && b.counts.length === 4);
    assert.strictEqual(b.labels.filter((l) => l >= 0).length, 119);
    assert.strictEqual(new Set(b.labels.filter((l) => l >= 0)).size, b.counts[0]);
    const again = await w.bodies();
    assert.deepStrictEqual(Array.from(again.labels), Array.from(b.labels));
    out.labels = Array.from(b.labels);
    out.counts = b.counts;
    out.secondCounts = again.counts;
    await w.destroy();
    out.ok = true;
    console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); console.log(JSON.stringify(out)); process.exit(1); });
