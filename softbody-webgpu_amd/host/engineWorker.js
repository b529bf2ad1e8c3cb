'use strict';
/**
 * Host driver of the native engine: the counterpart of /root/reference/src/engineWorker.ts
 * without the canvas / render pass / Worker thread.  Same state, same message protocol
 * (engineWorker.ts:490-545), same three locked operations:
 *   writeBuffers()  engineWorker.ts:580-597  ->  sb_write_buffers
 *   loadBuffers()   engineWorker.ts:548-579  ->  sb_load_buffers
 *   frame()         engineWorker.ts:626-695  ->  sb_write_user_input + sb_frame
 * and the picture of the render pass (engineWorker.ts:666-683) headless:
 *   render()        renderPPM of the state loadBuffers() would read  ->  sb_render (on the GPU, no read-back)
 */
const { WGPUSoftbodyEngineMessageTypes: MSG } = require('./messages');
const { BufferMapper, Vector2D } = require('./engineMapping');
const { AsyncLock } = require('./lock');
const { native, COLLIDE, PATH } = require('./native');

/** segments [[x0, y0, x1, y1], ...] then discs [[x, y, r], ...] as sb_cut_shape words: 8 per shape, kind 1 / 2, float32 bits */
function packCutShapes(segments, discs) {
    const n = segments.length + discs.length;
    const words = new Uint32Array(8 * n), floats = new Float32Array(words.buffer);
    segments.forEach((s, i) => {
        if (s.length !== 4) throw new RangeError('cut: a segment is [x0, y0, x1, y1]');
        words[8 * i] = 1;
        floats.set(s, 8 * i + 1);
    });
    discs.forEach((d, j) => {
        if (d.length !== 3) throw new RangeError('cut: a disc is [x, y, r]');
        const i = segments.length + j;
        words[8 * i] = 2;
        floats.set(d, 8 * i + 1);
    });
    return words;
}

class WGPUSoftbodyEngineWorker {
    static create(canvas, opts, post) {
        WGPUSoftbodyEngineWorker.sInstance = new WGPUSoftbodyEngineWorker(canvas, opts, post);
        return WGPUSoftbodyEngineWorker.sInstance;
    }
    static instance() { return WGPUSoftbodyEngineWorker.sInstance; }

    /**
     * @param canvas ignored (kept for signature compatibility; there is no render pass)
     * @param opts {particleRadius, subticks} as in the reference, plus {boundsSize, layout,
     *        maxParticles, maxBeams, collisionMode, path, tileParticles, device, gridSkin, blockSubsteps}
     * @param post function(message) receiving {type, data} replies
     */
    constructor(canvas, opts, post) {
        const o = opts || {};
        this.boundsSize = o.boundsSize !== undefined ? o.boundsSize : 1000;        // engineWorker.ts:39
        this.particleRadius = o.particleRadius !== undefined ? o.particleRadius : 10; // :40,89
        this.subticks = Math.ceil((o.subticks !== undefined ? o.subticks : 64) / 2) * 2; // :41,90
        this.layout = o.layout !== undefined ? o.layout : 1;
        this.lock = new AsyncLock();
        this.post = post || (() => {});
        this.addon = native();
        // capacity: the reference asks the adapter (engineWorker.ts:118-122); here the caller may size it
        const cap = o.maxByteLength !== undefined ? o.maxByteLength : (this.layout === 1 ? 1 << 27 : 1 << 31);
        this.bufferMapper = new BufferMapper(cap, { layout: this.layout, maxParticles: o.maxParticles, maxBeams: o.maxBeams });
        this.handle = this.addon.create({
            boundsSize: this.boundsSize, particleRadius: this.particleRadius, subticks: this.subticks,
            maxParticles: this.bufferMapper.maxParticles, maxBeams: this.bufferMapper.maxBeams, layout: this.layout,
            collisionMode: o.collisionMode !== undefined ? o.collisionMode : COLLIDE.GRID, // same bits as ALLPAIRS
            path: o.path !== undefined ? o.path : PATH.AUTO, tileParticles: o.tileParticles || 0, device: o.device || 0,
            gridSkin: o.gridSkin || 0, blockSubsteps: o.blockSubsteps || 0
        });
        this.running = true;
        this.visible = true;
        this.uploaded = false;
        this.frameTimes = [];
        this.userInput = { appliedForce: Vector2D.zero, mousePos: Vector2D.zero, lastMouse: Vector2D.zero,
            mouseActive: false, lastFrame: Date.now() };
    }

    get currentFps() { return this.frameTimes.length; }

    _buffers() {
        const m = this.bufferMapper;
        return [m.metadata, m.mapping, m.particleData, m.beamData];
    }

    /** device -> host ArrayBuffers of the BufferMapper (engineWorker.ts:548-579) */
    async loadBuffers() {
        await this.lock.run(() => {
            if (this.uploaded) this.addon.loadBuffers(this.handle, ...this._buffers());
        });
    }
    /** host ArrayBuffers -> device; also resets accumulators and the second particle buffer (:580-597) */
    async writeBuffers() {
        await this.lock.run(() => {
            this.addon.writeBuffers(this.handle, ...this._buffers());
            this.uploaded = true;
        });
    }

    /** one frame = user input upload + `subticks` substeps + one delete pass (:626-695, minus rendering) */
    async frame() {
        await this.lock.run(() => {
            if (!this.uploaded) return;
            const now = Date.now();
            const ui = this.userInput;
            const meta = this.bufferMapper.meta;
            meta.setUserInput(
                ui.appliedForce,
                ui.mousePos.mult(this.boundsSize),
                ui.mousePos.sub(ui.lastMouse).mult(this.currentFps * (now - ui.lastFrame) / 1000 * this.boundsSize),
                ui.mouseActive);
            meta.writeUserInput({ writeUserInput: (bytes) => this.addon.writeUserInput(this.handle, bytes) }, null);
            ui.lastMouse = ui.mousePos;
            ui.lastFrame = now;
            this.addon.frame(this.handle);
            this.addon.sync(this.handle); // device.queue.onSubmittedWorkDone(), :687
        });
        const t = Date.now();
        this.frameTimes.push(t);
        while (this.frameTimes[0] + 1000 < t) this.frameTimes.shift();
        this.post({ type: MSG.FRAMERATE, data: this.currentFps });
    }

    /**
     * The picture host/render.js renderPPM(mapper, opts) returns for the state loadBuffers() would read back, byte for byte
     * ("P6" header included), drawn on the GPU (sb_render): no state travels to the host.
     * @param opts {resolution (512), boundsSize, particleRadius} -- the engine's own bounds / radius unless given
     * @returns Buffer
     */
    async render(opts) {
        const o = opts || {};
        return this.lock.run(() => {
            if (!this.uploaded) throw new Error('render before writeBuffers');
            return this.addon.render(this.handle, {
                resolution: o.resolution || 512,
                boundsSize: o.boundsSize !== undefined ? o.boundsSize : this.boundsSize,
                particleRadius: o.particleRadius !== undefined ? o.particleRadius : this.particleRadius
            });
        });
    }

    /**
     * One row of 24 statistics of the whole scene (counts, means, extremes, kinetic energy: the words of sb_summary in
     * include/softbody.h), reduced on the GPU (sb_summary): no state travels to the host.
     * @param opts {partials} -- where the reduction is cut (the result does not depend on it)
     * @returns {row: Float32Array(24), counts: Float64Array(8)}
     */
    async summary(opts) {
        const o = opts || {};
        return this.lock.run(() => {
            if (!this.uploaded) throw new Error('summary before writeBuffers');
            return this.addon.summary(this.handle, { partials: o.partials || 0 });
        });
    }

    /**
     * The connected bodies of the whole scene -- particles joined by live beams; a pending break flag still connects, a beam a
     * delete pass removed does not -- labelled on the GPU (sb_bodies): no state travels to the host.
     * @returns {labels: Int32Array(maxParticles), counts: [bodies, particles of the largest, bodies of one particle, label of the
     *          largest]}; labels[i] is the smallest data index of the body of the particle at data index i, -1 where none lives
     */
    async bodies() {
        return this.lock.run(() => {
            if (!this.uploaded) throw new Error('bodies before writeBuffers');
            return this.addon.bodies(this.handle, this.bufferMapper.maxParticles);
        });
    }

    /**
     * Who touches whom, and who touches a wall, in the whole scene -- two particles touch iff the next substep's collision loop
     * would act on them -- found on the GPU (sb_contacts): no state travels to the host.
     * @param opts {pairs: rows of the pair list to return (default 0: none)}
     * @returns {touch: Int32Array(4 * maxParticles), counts: [pairs, -1, particles on a wall, particles touching another],
     *          pairs: Int32Array(2 * opts.pairs)}; touch holds per particle data index {partners, -1, wall bits, smallest
     *          partner or -1}; pairs the first opts.pairs pairs {i, j}, i < j, ascending, {-1, -1} behind the last
     */
    async contacts(opts) {
        return this.lock.run(() => {
            if (!this.uploaded) throw new Error('contacts before writeBuffers');
            return this.addon.contacts(this.handle, this.bufferMapper.maxParticles, (opts && opts.pairs) || 0);
        });
    }

    /**
     * Statistics per body of the whole scene, the same bits on every run -- found on the GPU (sb_body_summary) with the engine's
     * own bodies as the groups: no state travels to the host and no labels go through Node.
     * @param opts {rows: rows to return, 1 .. maxParticles (default 8, at most maxParticles)}
     * @returns {rows: Float32Array(24 * rows), counts: Float64Array(8 * rows), rank: Int32Array(maxParticles)}; row k is the body
     *          of rank k (particles descending, then label ascending; the empty row behind the last: label -1, counts 0, NaN
     *          elsewhere); counts holds per row the exact {particles, live beams, label, pending breaks, non-finite particles,
     *          non-finite beams, finite particles, 0}; rank[i] is the rank of the body of the particle at data index i, -1 where
     *          none lives
     */
    async bodySummary(opts) {
        return this.lock.run(() => {
            if (!this.uploaded) throw new Error('bodySummary before writeBuffers');
            const cap = this.bufferMapper.maxParticles;
            return this.addon.bodySummary(this.handle, cap, (opts && opts.rows) || Math.min(8, cap));
        });
    }

    /**
     * Cut the scene on the GPU (sb_cut): every live beam that a knife stroke crosses or an eraser disc covers -- the predicate of
     * include/softbody.h on the positions as they are now -- gets its pending break flag raised, as if it had broken in the last
     * substep; the next frame's delete pass removes it.  No state travels to the host.
     * @param opts {segments: [[x0, y0, x1, y1], ...], discs: [[x, y, r], ...] (at most 64 shapes together), dryRun: report only,
     *        hit: also return the hit bytes}
     * @returns {counts: Float64Array(4) [tested, hit, flagged, already flagged], hit?: Uint8Array(maxBeams)}; hit[d] is 1 where
     *          the beam at data index d was hit
     */
    async cut(opts) {
        const o = opts || {};
        const shapes = packCutShapes(o.segments || [], o.discs || []);
        return this.lock.run(() => {
            if (!this.uploaded) throw new Error('cut before writeBuffers');
            return this.addon.cut(this.handle, this.bufferMapper.maxBeams, shapes, !!o.dryRun, !!o.hit);
        });
    }

    /**
     * Keep a copy of everything a run mutates in device memory of the engine's (sb_checkpoint_device): one per engine, a later one
     * replaces it, every writeBuffers drops it.  No state travels to the host.
     */
    async checkpoint() {
        await this.lock.run(() => {
            if (!this.uploaded) throw new Error('checkpoint before writeBuffers');
            this.addon.checkpoint(this.handle);
        });
    }

    /**
     * Back to the checkpoint (sb_restore_device): every later frame, read-back and report gives the bits the engine gave, or would
     * have given, at and after checkpoint().  Physics constants and user input stay as they are now.  Rejects with the engine's
     * message when there is no checkpoint.
     */
    async restore() {
        await this.lock.run(() => {
            if (!this.uploaded) throw new Error('restore before writeBuffers');
            this.addon.restore(this.handle);
        });
    }

    /** benchmark granularity: n substeps, no delete pass; returns device milliseconds */
    async step(n) {
        return this.lock.run(() => this.addon.stepTimed(this.handle, n));
    }

    /** the message protocol of engineWorker.ts:490-545 */
    async onMessage(msg) {
        const mapper = this.bufferMapper;
        switch (msg.type) {
            case MSG.DESTROY:
                await this.destroy();
                break;
            case MSG.PHYSICS_CONSTANTS: {
                const c = Object.assign({}, msg.data, { gravity: Vector2D.fromObject(msg.data.gravity) });
                mapper.meta.setPhysicsConstants(c);
                // the reference reads back and re-uploads the whole scene here (:499-504); the C ABI
                // updates the 32 bytes in place, which leaves the same device state
                await this.lock.run(() => {
                    if (this.uploaded) this.addon.setPhysicsConstants(this.handle, mapper.meta.physicsConstantsArray());
                });
                this.post({ type: MSG.PHYSICS_CONSTANTS, data: mapper.meta.getPhysicsConstants() });
                break;
            }
            case MSG.GET_PHYSICS_CONSTANTS:
                await this.loadBuffers();
                this.post({ type: MSG.PHYSICS_CONSTANTS, data: mapper.meta.getPhysicsConstants() });
                break;
            case MSG.INPUT:
                this.userInput.appliedForce = Vector2D.fromObject(msg.data[0]);
                this.userInput.mousePos = Vector2D.fromObject(msg.data[1]);
                this.userInput.mouseActive = !!msg.data[2];
                this.post({ type: MSG.INPUT });
                break;
            case MSG.VISIBILITY_CHANGE:
                this.visible = !msg.data;
                break;
            case MSG.SNAPSHOT_SAVE:
                await this.loadBuffers();
                mapper.loadState();
                this.post({ type: MSG.SNAPSHOT_SAVE, data: mapper.createSnapshotBuffer() });
                break;
            case MSG.SNAPSHOT_LOAD: {
                const ok = mapper.loadSnapshotbuffer(msg.data);
                if (ok) await this.writeBuffers();
                this.post({ type: MSG.SNAPSHOT_LOAD, data: ok });
                break;
            }
            case MSG.CORRUPT_BUFFERS:
                // fault-injection toy of the web app (engineWorker.ts:599-617); not part of the physics path
                throw new Error('CORRUPT_BUFFERS is not supported by the native engine');
            default:
                break;
        }
    }

    async destroy() {
        if (!this.running) return;
        this.running = false;
        await this.lock.run(() => this.addon.destroy(this.handle));
        this.handle = null;
        this.post({ type: MSG.DESTROY });
        if (WGPUSoftbodyEngineWorker.sInstance === this) WGPUSoftbodyEngineWorker.sInstance = null;
    }
}
WGPUSoftbodyEngineWorker.sInstance = null;

module.exports = { WGPUSoftbodyEngineWorker };
