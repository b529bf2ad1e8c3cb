"""numpy restatement of host/render.js renderPPM (the picture sb_render draws), vectorised.

render_ref(buf, resolution, bounds_size, particle_radius) -> (res, res, 3) uint8, rows top to bottom: the PPM body of
renderPPM(mapper, {resolution, boundsSize, particleRadius}) for a mapper holding the four buffers of `buf` (a layout.Buffers).
Every JS number operation is restated in float64 in render.js's order (numpy does not contract a * b + c); Float32 data is read
as float32 and widened; colours go through a float32 store, clamp01 * 255 and Math.round; NaN components give byte 0.
Math.hypot is V8's (both arguments scaled by the larger magnitude, the squares summed with Kahan compensation).
Where render.js does not terminate (non-finite particle or beam endpoint coordinates, box bounds or point counts of 2^53 and
beyond) nothing is drawn for that primitive, as sb_render does (include/softbody.h).
"""
import numpy as np

TWO53 = 9007199254740992.0
_INNER = (0.0, 0.35, 0.5)
_RING = (1.0, 1.0, 1.0)


def v8_hypot(a, b):
    """V8's Math.hypot(a, b) on float64 arrays of finite values."""
    x, y = np.abs(a), np.abs(b)
    mx = np.maximum(x, y)
    safe = np.where(mx == 0.0, 1.0, mx)
    s = np.zeros_like(x)
    comp = np.zeros_like(x)
    for v in (x, y):
        n = v / safe
        summand = n * n - comp
        pre = s + summand
        comp = (pre - s) - summand
        s = pre
    return np.where(mx == 0.0, 0.0, np.sqrt(s) * mx)


def js_clamp01(v):
    """Math.max(0, Math.min(1, v)) with JS NaN propagation."""
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), np.nan, np.minimum(np.maximum(v, 0.0), 1.0))


def js_byte(f32):
    """Buffer byte of Math.round(clamp01(img[k]) * 255) for a Float32Array component."""
    v = js_clamp01(np.asarray(f32, dtype=np.float32).astype(np.float64))
    out = np.floor(np.where(np.isnan(v), 0.0, v) * 255.0 + 0.5)
    return out.astype(np.uint8)


def _beam_colours(strain, stress):
    sn = strain.astype(np.float64)
    ss = stress.astype(np.float64)
    r = js_clamp01(ss + 1.0)
    g = js_clamp01(1.0 - ss)
    b0 = 1.0 - np.abs(sn)
    b = np.where(np.isnan(b0), np.nan, np.maximum(b0, 0.0))
    with np.errstate(invalid="ignore"):
        return np.stack([js_byte(r.astype(np.float32)), js_byte(g.astype(np.float32)), js_byte(b.astype(np.float32))], axis=-1)


def _counts(buf):
    return buf.particle_count, buf.beam_count


def render_ref(buf, resolution=512, bounds_size=1000.0, particle_radius=10.0, max_work=400_000_000):
    res = int(resolution) or 512
    S, r = float(bounds_size), float(particle_radius)
    resf = float(res)
    P, B = _counts(buf)
    maxP = buf.max_particles
    mapping = np.asarray(buf.mapping).astype(np.int64)
    pf = np.asarray(buf.particles, dtype=np.float32).reshape(-1, 6)
    npix = res * res
    # per pixel: the draw number of the last primitive that put it (-1: none) and its colour
    last = np.full(npix, -1, dtype=np.int64)

    def put(px, py, draw):
        """px, py: float64 integer coordinates; draw: int64 draw numbers (increasing in render.js order)."""
        ok = (px >= 0) & (py >= 0) & (px < resf) & (py < resf)
        px, py, draw = px[ok].astype(np.int64), py[ok].astype(np.int64), draw[ok]
        k = (res - 1 - py) * res + px
        np.maximum.at(last, k, draw)

    to_px = lambda v: v / S * resf  # noqa: E731

    # ---- particles: draw number 2 * slot + ring (a slot puts a pixel at most once)
    inner_b = js_byte(np.array(_INNER, dtype=np.float32))
    ring_b = js_byte(np.array(_RING, dtype=np.float32))
    if P:
        idx = mapping[:P]
        cx = pf[idx, 0].astype(np.float64)
        cy = pf[idx, 1].astype(np.float64)
        fin = np.isfinite(cx) & np.isfinite(cy)
        with np.errstate(invalid="ignore", over="ignore"):
            x0 = np.floor(to_px(cx - r))
            x1 = np.ceil(to_px(cx + r))
            y0 = np.floor(to_px(cy - r))
            y1 = np.ceil(to_px(cy + r))
        ok = fin & (y0 <= y1) & (np.abs(y0) < TWO53) & (np.abs(y1) < TWO53) & (x0 <= x1) & (np.abs(x0) < TWO53) & (np.abs(x1) < TWO53)
        cx0 = np.maximum(x0, 0.0)
        cx1 = np.minimum(x1, resf - 1)
        cy0 = np.maximum(y0, 0.0)
        cy1 = np.minimum(y1, resf - 1)
        ok &= (cx0 <= cx1) & (cy0 <= cy1)
        sl = np.nonzero(ok)[0]
        w = (cx1[sl] - cx0[sl] + 1).astype(np.int64)
        h = (cy1[sl] - cy0[sl] + 1).astype(np.int64)
        assert int((w * h).sum()) <= max_work, "render_ref: too many particle pixels"
        r08 = r * 0.8
        for (ww, hh) in sorted(set(zip(w.tolist(), h.tolist()))):
            grp = sl[(w == ww) & (h == hh)]
            step = max(1, 4_000_000 // (ww * hh))
            for g0 in range(0, len(grp), step):
                g = grp[g0:g0 + step]
                ox, oy = np.meshgrid(np.arange(ww, dtype=np.float64), np.arange(hh, dtype=np.float64))
                px = cx0[g][:, None] + ox.ravel()[None, :]
                py = cy0[g][:, None] + oy.ravel()[None, :]
                wx = (px + 0.5) / resf * S
                wy = (py + 0.5) / resf * S
                d = v8_hypot(wx - cx[g][:, None], wy - cy[g][:, None])
                ring = ~(d < r08) & (d < r)
                hit = (d < r08) | ring
                draw = (2 * g[:, None] + ring.astype(np.int64))
                draw = np.broadcast_to(draw, px.shape)
                put(px[hit], py[hit], draw[hit])

    # ---- beams: draw number 2 * P + slot
    beam_cols = np.zeros((0, 3), dtype=np.uint8)
    if B:
        bi = mapping[maxP:maxP + B]
        rec = buf.beams[bi]
        a = rec["a"].astype(np.int64)
        b = rec["b"].astype(np.int64)
        beam_cols = _beam_colours(rec["strain"], rec["stress"])
        with np.errstate(invalid="ignore", over="ignore"):
            ax = to_px(pf[a, 0].astype(np.float64))
            ay = to_px(pf[a, 1].astype(np.float64))
            bx = to_px(pf[b, 0].astype(np.float64))
            by = to_px(pf[b, 1].astype(np.float64))
            fin = np.isfinite(ax) & np.isfinite(ay) & np.isfinite(bx) & np.isfinite(by)
            dx = bx - ax
            dy = by - ay
            n = np.maximum(1.0, np.ceil(np.maximum(np.abs(dx), np.abs(dy))))
        ok = fin & (n < TWO53)
        sl = np.nonzero(ok)[0]
        cnt = (n[sl] + 1).astype(np.int64)
        assert int(cnt.sum()) <= max_work, "render_ref: too many beam points"
        chunk = 4_000_000
        start = 0
        cum = np.cumsum(cnt)
        while start < len(sl):
            base = cum[start - 1] if start else 0
            stop = int(np.searchsorted(cum, base + chunk, side="right"))
            stop = max(stop, start + 1)
            g = sl[start:stop]
            c = cnt[start:stop]
            rep = np.repeat(np.arange(len(g)), c)
            k = (np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)).astype(np.float64)
            gg = g[rep]
            px = np.floor(ax[gg] + dx[gg] * k / n[gg])
            py = np.floor(ay[gg] + dy[gg] * k / n[gg])
            put(px, py, 2 * P + gg.astype(np.int64))
            start = stop

    out = np.zeros((npix, 3), dtype=np.uint8)
    drawn = last >= 0
    lp = last[drawn]
    cols = np.empty((len(lp), 3), dtype=np.uint8)
    is_p = lp < 2 * P
    cols[is_p] = np.where((lp[is_p] & 1)[:, None] == 1, ring_b[None, :], inner_b[None, :])
    cols[~is_p] = beam_cols[lp[~is_p] - 2 * P]
    out[drawn] = cols
    return out.reshape(res, res, 3)


def ppm(body):
    """The P6 file renderPPM returns, from a (res, res, 3) body."""
    res = body.shape[0]
    return ("P6\n%d %d\n255\n" % (res, res)).encode("ascii") + body.tobytes()
