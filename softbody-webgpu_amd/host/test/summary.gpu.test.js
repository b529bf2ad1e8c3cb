'use strict';
// GPU test of the summary row through the Node path: JS host -> N-API addon -> sb_summary.  The row and the counts the worker /
// facade summary() return for the default scene after one frame are printed as words; tests/test_gpu_summary.py compares them with
// the bytes Python's Engine.summary_host() gives for the same scene and capacity.
const assert = require('assert');
const h = require('..');

const out = { ok: false };

(async () => {
    const w = new h.WGPUSoftbodyEngineWorker(null, { layout: 1, maxParticles: 128, maxBeams: 320, boundsSize: 1000, particleRadius: 10,
        subticks: 64, collisionMode: h.COLLIDE.OFF });
    h.defaultScene(w.bufferMapper);
    w.bufferMapper.writeState();
    await assert.rejects(w.summary(), /before writeBuffers/);
    await w.writeBuffers();
    await w.frame();
    const s = await w.summary();
    assert.ok(s.row instanceof Float32Array && s.row.length === 24);
    assert.ok(s.counts instanceof Float64Array && s.counts.length === 8);
    assert.strictEqual(s.row[0], s.counts[0]);
    assert.strictEqual(s.row[20], 1);
    const cut = await w.summary({ partials: 256 });
    assert.deepStrictEqual(Array.from(new Uint32Array(cut.row.buffer)), Array.from(new Uint32Array(s.row.buffer)));
    await assert.rejects(w.summary({ partials: 300 }));
    out.row = Array.from(new Uint32Array(s.row.buffer));
    out.counts = Array.from(s.counts);
    out.workerCounts = Array.from(cut.counts);
    await w.destroy();
    out.ok = true;
    console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); console.log(JSON.stringify(out)); process.exit(1); });
