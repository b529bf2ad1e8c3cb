'use strict';
// renderPPM of four raw buffer files (tests/test_render_ref_cpu.py: the numpy restatement tests/render_ref.py against render.js).
// node render_dump.js <job.json>   job = { dir, layout, maxParticles, particleCount, beamCount, resolution, boundsSize,
//                                          particleRadius, out }; dir holds mapping.bin, particles.bin, beams.bin
const fs = require('fs');
const path = require('path');
const { LAYOUTS } = require('../engineMapping');
const { renderPPM } = require('../render');

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const rd = (f) => { const b = fs.readFileSync(path.join(job.dir, f)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); };
const mapper = {
    layout: LAYOUTS[job.layout], mapping: rd('mapping.bin'), particleData: rd('particles.bin'), beamData: rd('beams.bin'),
    maxParticles: job.maxParticles, meta: { particleCount: job.particleCount, beamCount: job.beamCount }
};
const o = { resolution: job.resolution };
if (job.boundsSize !== undefined) o.boundsSize = job.boundsSize;
if (job.particleRadius !== undefined) o.particleRadius = job.particleRadius;
fs.writeFileSync(job.out, renderPPM(mapper, o));
console.log(JSON.stringify({ ok: true }));
