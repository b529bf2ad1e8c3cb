'use strict';
// GPU test of the halo guard FROM THE NODE HOST (tests/test_gpu_halo_guard_node.py): partitionScene hands out the guard data
// (held masks agree with the plan lists), and two guarded PeerExchangers -- two engines of this process, each on its slab of two
// clouds of free particles that fly at each other -- throw RepartitionDueError once the clouds enter each other's slabs.  The
// same scene with collisions off (only checks C and D apply) runs through without a throw.  Addon errors: haloGuardStatus
// without a guard, haloGuard before haloConfigure.
const assert = require('assert');
const h = require('..');

const DEPTH = 1, REACH = 130, SUBTICKS = 64; // R >= 3C = 3 * depth * (H + H / 16), H = 1.5 * 2r = 30

function clouds() {
    const m = new h.BufferMapper(1 << 22, { layout: 2, maxParticles: 256, maxBeams: 16 });
    let id = 0;
    for (const [cx, vx] of [[250, 20], [750, -20]])
        for (let i = 0; i < 10; i++)
            for (let j = 0; j < 12; j++) {
                const u = Math.sin(id * 12.9898) * 3, w = Math.cos(id * 78.233) * 3;
                m.addParticle(new h.Particle(id++, new h.Vector2D(cx - 150 + 30 * i + u, 40 + 30 * j + w), new h.Vector2D(vx + u / 2, w / 2)));
            }
    m.writeState();
    return m;
}

async function ranks(mode, guard) {
    const made = h.partitionScene(clouds(), 2, DEPTH, REACH);
    const ws = [], exs = [];
    for (const local of made) {
        const w = new h.WGPUSoftbodyEngineWorker(null, { layout: 2, boundsSize: 1000, maxParticles: local.maxParticles,
            maxBeams: local.maxBeams, collisionMode: mode });
        for (const k of ['metadata', 'mapping', 'particleData', 'beamData']) new Uint8Array(w.bufferMapper[k]).set(new Uint8Array(local[k]));
        await w.writeBuffers();
        ws.push(w);
        exs.push(new h.PeerExchanger(w.handle, local.plan, { guard, timeoutMs: 3000 }));
    }
    const cards = exs.map((ex) => ex.card);
    exs.forEach((ex) => ex.connect(cards));
    return { made, ws, exs };
}

(async () => {
    const out = { ok: false };
    // guard data of the partition
    const made = h.partitionScene(clouds(), 2, DEPTH, REACH);
    const holders = made.map((l) => new Set(Array.from(l.plan.globalParticleId)));
    for (const l of made) {
        const g = l.plan.guard;
        assert.ok(g && g.lo.length === 2 && g.held.length === l.plan.nLocal && g.reach === REACH && Math.abs(g.hop - 30) < 1e-6);
        l.plan.globalParticleId.forEach((gid, i) => {
            let want = 0n;
            holders.forEach((s, t) => { if (s.has(gid)) want |= 1n << BigInt(t); });
            assert.strictEqual(g.held[i], want);
        });
    }
    // collisions on: the clouds make the partition stale -> RepartitionDueError with its fields
    let r = await ranks(h.COLLIDE.ALLPAIRS, true);
    let thrown = null;
    for (let f = 0; f < 9 && !thrown; f++)
        for (const ex of r.exs) {
            try { ex.frame(SUBTICKS); } catch (e) { if (!(e instanceof h.RepartitionDueError)) throw e; thrown = thrown || { f, e }; }
        }
    assert.ok(thrown, 'the guard never fired');
    const e = thrown.e, plan = r.made[e.rank].plan;
    assert.ok((e.kinds & 3) && e.kindNames.length && e.violations > 0 && e.refresh !== null && e.isBeam === false);
    assert.ok(Array.from(plan.ownedParticles).some((i) => plan.globalParticleId[i] === e.globalId));
    const st = r.exs[e.rank].guardStatus();
    assert.strictEqual(st.kinds, e.kinds);
    assert.strictEqual(st.refreshes, (thrown.f + 1) * SUBTICKS);
    out.fired = { frame: thrown.f, rank: e.rank, kinds: e.kindNames, refresh: e.refresh, globalId: e.globalId };
    for (const w of r.ws) await w.destroy();
    // collisions off: only C and D apply, the clouds pass through each other quietly
    r = await ranks(h.COLLIDE.OFF, true);
    for (let f = 0; f < 9; f++) for (const ex of r.exs) ex.frame(SUBTICKS);
    for (const ex of r.exs) assert.strictEqual(ex.guardStatus().kinds, 0);
    out.quietRefreshes = r.exs[0].guardStatus().refreshes;
    // errors: status without a guard, guard before haloConfigure
    const a = h.native(), w = r.ws[0];
    a.haloGuard(w.handle, null);
    assert.throws(() => a.haloGuardStatus(w.handle), /without a guard/);
    for (const x of r.ws) await x.destroy();
    const fresh = new h.WGPUSoftbodyEngineWorker(null, { layout: 2, boundsSize: 1000, maxParticles: made[0].maxParticles,
        maxBeams: made[0].maxBeams, collisionMode: h.COLLIDE.ALLPAIRS });
    for (const k of ['metadata', 'mapping', 'particleData', 'beamData']) new Uint8Array(fresh.bufferMapper[k]).set(new Uint8Array(made[0][k]));
    await fresh.writeBuffers();
    const g = made[0].plan.guard, own = made[0].plan.ownedParticles;
    const desc = { rank: 0, world: 2, depth: DEPTH, contactReach: REACH, hop: g.hop, ownParticles: own,
        held: BigUint64Array.from(own, (i) => g.held[i]), ownBeams: made[0].plan.ownedBeams, lo: g.lo, hi: g.hi };
    assert.throws(() => a.haloGuard(fresh.handle, desc), /before sb_halo_configure/);
    assert.throws(() => a.haloGuard(fresh.handle, Object.assign({}, desc, { held: new BigUint64Array(0) })), TypeError);
    assert.throws(() => new h.PeerExchanger(fresh.handle, Object.assign(Object.create(Object.getPrototypeOf(made[0].plan)), made[0].plan, { guard: null }), { guard: true }), TypeError);
    await fresh.destroy();
    out.ok = true;
    console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
