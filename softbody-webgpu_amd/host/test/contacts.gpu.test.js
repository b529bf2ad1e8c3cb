'use strict';
// GPU test of the contacts through the Node path: JS host -> N-API addon -> sb_contacts.  The touch rows, the counts and the pair
// list the worker / facade contacts() return for the default scene after one frame are printed; tests/test_gpu_contacts.py compares
// them with what Python's Engine.contacts_host() gives for the same scene and capacity.
const assert = require('assert');
const h = require('..');

const out = { ok: false };

(async () => {
    const w = new h.WGPUSoftbodyEngineWorker(null, { layout: 1, maxParticles: 128, maxBeams: 320, boundsSize: 1000, particleRadius: 10,
        subticks: 64, collisionMode: h.COLLIDE.GRID });
    h.defaultScene(w.bufferMapper);
    w.bufferMapper.writeState();
    await assert.rejects(w.contacts(), /before writeBuffers/);
    await w.writeBuffers();
    await w.frame();
    const c = await w.contacts({ pairs: 64 });
    assert.ok(c.touch instanceof Int32Array && c.touch.length === 4 * 128);
    assert.ok(c.pairs instanceof Int32Array && c.pairs.length === 2 * 64);
    assert.ok(Array.isArray(c.counts) && c.counts.length === 4 && c.counts[1] === -1);
    const none = await w.contacts();
    assert.strictEqual(none.pairs.length, 0);
    assert.deepStrictEqual(Array.from(none.touch), Array.from(c.touch));
    out.touch = Array.from(c.touch);
    out.pairs = Array.from(c.pairs);
    out.counts = c.counts;
    out.secondCounts = none.counts;
    await w.destroy();
    out.ok = true;
    console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); console.log(JSON.stringify(out)); process.exit(1); });
