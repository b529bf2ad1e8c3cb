'use strict';
// GPU test of checkpoint / restore through the Node path: JS host -> N-API addon -> sb_checkpoint_device / sb_restore_device.
// Two workers run the default scene: one straight, one that checkpoints after two frames, runs three more, restores and runs on.
// The read-backs (all four buffers) must be equal byte for byte at the restore and at the end; the same through the facade.
const assert = require('assert');
const h = require('..');

const out = { ok: false };
const OPTS = { layout: 1, maxParticles: 128, maxBeams: 320, boundsSize: 1000, particleRadius: 10, subticks: 64 };

async function state(w) {
    await w.loadBuffers();
    const m = w.bufferMapper;
    return [m.metadata, m.mapping, m.particleData, m.beamData].map((b) => Buffer.from(b.slice(0)));
}
function same(a, b, what) {
    for (let i = 0; i < 4; i++) assert.ok(a[i].equals(b[i]), what + ': buffer ' + i + ' differs');
}
async function frames(w, n) { for (let i = 0; i < n; i++) await w.frame(); }
function worker(collisionMode) {
    const w = new h.WGPUSoftbodyEngineWorker(null, Object.assign({ collisionMode }, OPTS));
    h.defaultScene(w.bufferMapper);
    w.bufferMapper.writeState();
    return w;
}

(async () => {
    for (const mode of [h.COLLIDE.OFF, h.COLLIDE.GRID]) {
        const n = worker(mode), c = worker(mode);
        await assert.rejects(c.checkpoint(), /before writeBuffers/);
        await assert.rejects(c.restore(), /before writeBuffers/);
        await n.writeBuffers();
        await c.writeBuffers();
        await assert.rejects(c.restore(), /SB_ERR_STATE|without a checkpoint/);   // the engine's message
        await frames(n, 2);
        await frames(c, 2);
        await c.checkpoint();
        const atCheckpoint = await state(c);
        await frames(c, 3);
        const ranOn = await state(c);
        assert.ok(!ranOn[2].equals(atCheckpoint[2]), 'three frames must move the particles');
        await c.restore();
        same(await state(c), atCheckpoint, 'right after the restore');
        same(await state(n), atCheckpoint, 'the straight run at the checkpoint');
        await frames(c, 3);
        same(await state(c), ranOn, 'the same three frames again');
        await frames(n, 5);
        await frames(c, 2);
        same(await state(c), await state(n), 'rewound vs straight, 7 frames');
        await c.writeBuffers();                                                  // every upload drops the checkpoint
        await assert.rejects(c.restore(), /SB_ERR_STATE|without a checkpoint/);
        out.restores = (out.restores || 0) + c.addon.getInfo(c.handle, 'restores');
        await n.destroy();
        await c.destroy();
    }
    // the facade
    const e = new h.WGPUSoftbodyEngine(Object.assign({ collisionMode: h.COLLIDE.GRID }, OPTS));
    h.defaultScene(e.worker.bufferMapper);
    e.worker.bufferMapper.writeState();
    await e.worker.writeBuffers();
    await e.run(1);
    await e.checkpoint();
    const a = await state(e.worker);
    await e.run(2);
    await e.restore();
    same(await state(e.worker), a, 'facade');
    await e.destroy();
    out.ok = true;
    console.log(JSON.stringify(out));
})().catch((err) => { console.error(err); console.log(JSON.stringify(out)); process.exit(1); });
