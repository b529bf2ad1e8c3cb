'use strict';
// GPU test of the per-body statistics through the Node path: JS host -> N-API addon -> sb_body_summary.  The rows (as their bits),
// the exact counts and the ranks the worker / facade bodySummary() return for the default scene after one frame are printed;
// tests/test_gpu_body_summary.py compares them with what Python's Engine.body_summary_host() gives for the same scene and capacity.
const assert = require('assert');
const h = require('..');

const out = { ok: false };

(async () => {
    const w = new h.WGPUSoftbodyEngineWorker(null, { layout: 1, maxParticles: 128, maxBeams: 320, boundsSize: 1000, particleRadius: 10,
        subticks: 64, collisionMode: h.COLLIDE.OFF });
    h.defaultScene(w.bufferMapper);
    w.bufferMapper.writeState();
    await assert.rejects(w.bodySummary(), /before writeBuffers/);
    await w.writeBuffers();
    await w.frame();
    const s = await w.bodySummary({ rows: 12 });
    assert.ok(s.rows instanceof Float32Array && s.rows.length === 24 * 12);
    assert.ok(s.counts instanceof Float64Array && s.counts.length === 8 * 12);
    assert.ok(s.rank instanceof Int32Array && s.rank.length === 128);
    const d = await w.bodySummary();
    assert.strictEqual(d.rows.length, 24 * 8);
    assert.deepStrictEqual(Array.from(new Uint32Array(d.rows.buffer, d.rows.byteOffset, 24 * 8)),
        Array.from(new Uint32Array(s.rows.buffer, s.rows.byteOffset, 24 * 8)));
    assert.deepStrictEqual(Array.from(d.rank), Array.from(s.rank));
    await assert.rejects(w.bodySummary({ rows: 129 }), /rows must be/);
    out.rowBits = Array.from(new Uint32Array(s.rows.buffer, s.rows.byteOffset, s.rows.length));
    out.counts = Array.from(s.counts);
    out.rank = Array.from(s.rank);
    await w.destroy();
    out.ok = true;
    console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); console.log(JSON.stringify(out)); process.exit(1); });
