'use strict';
// GPU test of cutting through the Node path: JS host -> N-API addon -> sb_cut.  One knife stroke across the default scene's long
// 20 x 2 strip (x = 685 lies between its columns 9 and 10), plus a disc over the 9 x 4 blob: the counts and the hit bytes must
// equal a restatement of the predicate of include/softbody.h in JS with Math.fround after every operator, and after the frame
// that removes the hit beams the strip is two bodies.  The result is printed for tests/test_gpu_cut.py.
const assert = require('assert');
const h = require('..');

const f = Math.fround;
const orient = (u, v, w) => f(f(f(v[0] - u[0]) * f(w[1] - u[1])) - f(f(v[1] - u[1]) * f(w[0] - u[0])));
const inbox = (u, v, w) => Math.min(u[0], v[0]) <= w[0] && w[0] <= Math.max(u[0], v[0]) && Math.min(u[1], v[1]) <= w[1] && w[1] <= Math.max(u[1], v[1]);
function segmentHits(P, Q, A, B) {
    const d1 = orient(P, Q, A), d2 = orient(P, Q, B), d3 = orient(A, B, P), d4 = orient(A, B, Q);
    if (((d1 > 0 && d2 < 0) || (d1 < 0 && d2 > 0)) && ((d3 > 0 && d4 < 0) || (d3 < 0 && d4 > 0))) return true;
    return (d1 === 0 && inbox(P, Q, A)) || (d2 === 0 && inbox(P, Q, B)) || (d3 === 0 && inbox(A, B, P)) || (d4 === 0 && inbox(A, B, Q));
}
function discHits(C, r, A, B) {
    if (!(r >= 0)) return false;
    const d = [f(B[0] - A[0]), f(B[1] - A[1])], w = [f(C[0] - A[0]), f(C[1] - A[1])];
    const L2 = f(f(d[0] * d[0]) + f(d[1] * d[1])), t = f(f(w[0] * d[0]) + f(w[1] * d[1])), r2 = f(r * r);
    if (!(t > 0)) return f(f(w[0] * w[0]) + f(w[1] * w[1])) <= r2;
    if (t >= L2) {
        const u = [f(C[0] - B[0]), f(C[1] - B[1])];
        return f(f(u[0] * u[0]) + f(u[1] * u[1])) <= r2;
    }
    const c = f(f(d[0] * w[1]) - f(d[1] * w[0]));
    return f(c * c) <= f(r2 * L2);
}

const out = { ok: false };

(async () => {
    const maxP = 128, maxB = 320;
    const w = new h.WGPUSoftbodyEngineWorker(null, { layout: 2, maxParticles: maxP, maxBeams: maxB, boundsSize: 1000, particleRadius: 10,
        subticks: 64, collisionMode: h.COLLIDE.OFF });
    h.defaultScene(w.bufferMapper);
    w.bufferMapper.writeState();
    const segments = [[685, 0, 685, 100]], discs = [[150, 165, 40]];
    await assert.rejects(w.cut({ segments }), /before writeBuffers/);
    await w.writeBuffers();
    // the restatement, on the uploaded buffers (layout 2: u32 mapping, beam record = u32 a, u32 b, 9 f32)
    const bm = w.bufferMapper, nb = bm.meta.beamCount;
    const map = new Uint32Array(bm.mapping), pos = new Float32Array(bm.particleData), rec = new Uint32Array(bm.beamData);
    const want = new Uint8Array(maxB);
    let hits = 0;
    for (let s = 0; s < nb; s++) {
        const d = map[maxP + s], a = rec[11 * d], b = rec[11 * d + 1];
        const A = [pos[6 * a], pos[6 * a + 1]], B = [pos[6 * b], pos[6 * b + 1]];
        const hit = segments.some((g) => segmentHits([f(g[0]), f(g[1])], [f(g[2]), f(g[3])], A, B)) ||
            discs.some((c) => discHits([f(c[0]), f(c[1])], f(c[2]), A, B));
        want[d] = hit ? 1 : 0;
        hits += hit ? 1 : 0;
    }
    assert.ok(hits > 0 && hits < nb);
    const before = await w.bodies();
    const dry = await w.cut({ segments, discs, dryRun: true, hit: true });
    assert.ok(dry.counts instanceof Float64Array && dry.counts.length === 4 && dry.hit instanceof Uint8Array && dry.hit.length === maxB);
    assert.deepStrictEqual(Array.from(dry.counts), [nb, hits, 0, 0]);
    assert.deepStrictEqual(Array.from(dry.hit), Array.from(want));
    const eng = await w.cut({ segments, discs });
    assert.strictEqual(eng.hit, undefined);
    assert.deepStrictEqual(Array.from(eng.counts), [nb, hits, hits, 0]);
    const again = await w.cut({ segments, discs, hit: true });
    assert.deepStrictEqual(Array.from(again.counts), [nb, hits, 0, hits]);
    assert.deepStrictEqual(Array.from(again.hit), Array.from(want));
    assert.deepStrictEqual((await w.bodies()).counts, before.counts, 'a pending flag still connects');
    await w.frame();
    const after = await w.bodies();
    // the strip's particles: one body before, two after (its columns 0 .. 9 and 10 .. 19)
    const strip = [];
    for (let i = 0; i < bm.meta.particleCount; i++) if (pos[6 * i] >= 400 && pos[6 * i] <= 970 && pos[6 * i + 1] >= 40 && pos[6 * i + 1] <= 70) strip.push(i);
    assert.strictEqual(strip.length, 40);
    assert.strictEqual(new Set(strip.map((i) => before.labels[i])).size, 1);
    assert.strictEqual(new Set(strip.map((i) => after.labels[i])).size, 2);
    assert.ok(after.counts[0] > before.counts[0]);
    await assert.rejects(w.cut({ segments: new Array(65).fill(segments[0]) }), /sb_cut failed/);
    out.counts = Array.from(eng.counts);
    out.hit = Array.from(want);
    out.bodiesBefore = before.counts[0];
    out.bodiesAfter = after.counts[0];
    await w.destroy();
    out.ok = true;
    console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); console.log(JSON.stringify(out)); process.exit(1); });
