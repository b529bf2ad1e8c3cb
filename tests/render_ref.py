"""numpy restatement of host/render.js renderPPM (the picture sb_render draws), vectorised.

render_ref(buf, resolution, bounds_size, particle_radius) -> (res, res, 3) uint8, rows top to bottom: the PPM body of
renderPPM(mapper, {resolution, boundsSize, particleRadius}) for a mapper holding the four buffers of `buf` (a layout.Buffers).
Every JS number operation is restated in float64 in render.js's order (numpy does not contract a * b + c); Float32 data is read
as float32 and widened; colours go through a float32 store, clamp01 * 255 and Math.round; NaN components give byte 0.
Math.hypot is V8's (both arguments scaled by the larger magnitude, the squares summed with Kahan compensation).
Where render.js does not terminate (non-finite particle or beam endpoint coordinates, box bounds or point counts of 2^53 and
beyond) nothing is drawn for that primitive, as sb_render does (include/softbody.h).

Beams take one of two routes.  Up to WINDOW_THRESHOLD points every k of 0 .. n is evaluated (the enumerating route).  Longer beams
take the window route: on the major axis (the larger |d|; the coordinate moves at most a pixel per k there) the k at which the exact
line a + d k / n enters and leaves [0, res) are found in rational arithmetic, widened by WINDOW_MARGIN points and clamped to
0 .. n, and render.js's own float64 expression is evaluated on every k of that window.  Each window end that was not clamped is
asserted to lie outside the image on its side; every rounded operation of the expression is monotone in k, so no k outside the
window can land inside the image.  No bisection: the route shares nothing with the kernels' clip.  beam_route="enumerate" /
"window" forces one route for every beam (n = 1 and a major-axis d of 0 always enumerate).
"""
import math
from fractions import Fraction

import numpy as np

WINDOW_THRESHOLD = 4_000_000   # points; beams with more take the window route
WINDOW_MARGIN = 256            # points each window end is widened by (the float64 expression is within ~3 px of the exact line)

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


def particle_boxes(buf, resolution=512, bounds_size=1000.0, particle_radius=10.0):
    """Per particle slot: render.js's box (x0, x1, y0, y1: float64, before clipping), whether anything of it is walked (`ok`) and
    the pixels of the clipped box (0 where not ok): a dict of arrays."""
    res = int(resolution) or 512
    S, r, resf = float(bounds_size), float(particle_radius), float(res)
    P = buf.particle_count
    pf = np.asarray(buf.particles, dtype=np.float32).reshape(-1, 6)
    idx = np.asarray(buf.mapping).astype(np.int64)[:P]
    cx = pf[idx, 0].astype(np.float64)
    cy = pf[idx, 1].astype(np.float64)
    fin = np.isfinite(cx) & np.isfinite(cy)
    with np.errstate(invalid="ignore", over="ignore"):
        x0 = np.floor((cx - r) / S * resf)
        x1 = np.ceil((cx + r) / S * resf)
        y0 = np.floor((cy - r) / S * resf)
        y1 = np.ceil((cy + r) / S * resf)
        ok = fin & (y0 <= y1) & (np.abs(y0) < TWO53) & (np.abs(y1) < TWO53) & (x0 <= x1) & (np.abs(x0) < TWO53) & (np.abs(x1) < TWO53)
        cx0 = np.maximum(x0, 0.0)
        cx1 = np.minimum(x1, resf - 1)
        cy0 = np.maximum(y0, 0.0)
        cy1 = np.minimum(y1, resf - 1)
        ok &= (cx0 <= cx1) & (cy0 <= cy1)
    pixels = np.zeros(P, np.int64)
    pixels[ok] = ((cx1[ok] - cx0[ok] + 1) * (cy1[ok] - cy0[ok] + 1)).astype(np.int64)
    return dict(cx=cx, cy=cy, x0=x0, x1=x1, y0=y0, y1=y1, ok=ok, cx0=cx0, cx1=cx1, cy0=cy0, cy1=cy1, pixels=pixels)


def _beam_lines(buf, res, S):
    """render.js's numbers per beam slot: ax, ay, dx, dy, n (float64) and ok (it terminates); plus the records."""
    P, B = _counts(buf)
    resf = float(res)
    maxP = buf.max_particles
    mapping = np.asarray(buf.mapping).astype(np.int64)
    pf = np.asarray(buf.particles, dtype=np.float32).reshape(-1, 6)
    rec = buf.beams[mapping[maxP:maxP + B]]
    a = rec["a"].astype(np.int64)
    b = rec["b"].astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        ax = pf[a, 0].astype(np.float64) / S * resf
        ay = pf[a, 1].astype(np.float64) / S * resf
        bx = pf[b, 0].astype(np.float64) / S * resf
        by = pf[b, 1].astype(np.float64) / S * resf
        fin = np.isfinite(ax) & np.isfinite(ay) & np.isfinite(bx) & np.isfinite(by)
        dx = bx - ax
        dy = by - ay
        n = np.maximum(1.0, np.ceil(np.maximum(np.abs(dx), np.abs(dy))))
        ok = fin & (n < TWO53)
    return dict(rec=rec, ax=ax, ay=ay, dx=dx, dy=dy, n=n, ok=ok)


def _windowed(dx, dy, n, route):
    """Whether a beam that terminates takes the window route."""
    if n == 1.0 or max(abs(dx), abs(dy)) == 0.0 or route == "enumerate":
        return False
    return route == "window" or n + 1 > WINDOW_THRESHOLD


def _window(ax, ay, dx, dy, n, res):
    """The window route's k range [lo, hi] (Python ints; lo > hi: no point can be inside), its ends asserted."""
    N = int(n)
    a0, d = (ax, dx) if abs(dx) >= abs(dy) else (ay, dy)
    fa, fd = Fraction(a0), Fraction(d)
    t0, t1 = (0 - fa) * N / fd, (res - fa) * N / fd     # the exact line is at 0 and at res there
    if t0 > t1:
        t0, t1 = t1, t0
    lo_u = int(math.floor(t0)) - WINDOW_MARGIN
    hi_u = int(math.ceil(t1)) + WINDOW_MARGIN

    def side(k):
        """-1: the point of k is before the image on the major axis (in the direction of travel), +1: past it, 0: inside."""
        c = np.floor(a0 + d * float(k) / n)
        below, above = c < 0.0, c > float(res - 1)
        if not (below or above):
            return 0
        return -1 if (below if d > 0 else above) else 1

    if lo_u > N:
        assert side(N) == -1, "render_ref window: the last point is not before the image (widen WINDOW_MARGIN)"
        return 0, -1
    if hi_u < 0:
        assert side(0) == 1, "render_ref window: the first point is not past the image (widen WINDOW_MARGIN)"
        return 0, -1
    if lo_u > 0:
        assert side(lo_u) == -1, "render_ref window: the lower end is not before the image (widen WINDOW_MARGIN)"
    if hi_u < N:
        assert side(hi_u) == 1, "render_ref window: the upper end is not past the image (widen WINDOW_MARGIN)"
    return max(lo_u, 0), min(hi_u, N)


def _k_chunks(lo, hi, chunk=4_000_000):
    """float64 arrays of the integers lo .. hi (exact below 2^53)."""
    k = lo
    while k <= hi:
        e = min(hi, k + chunk - 1)
        yield np.arange(k, e + 1, dtype=np.int64).astype(np.float64)
        k = e + 1


def beam_spans(buf, resolution=512, bounds_size=1000.0, beam_route=None, max_work=400_000_000):
    """Per beam slot a dict: n (float64; None where render.js's n is not finite), drawn (it terminates), windowed, count (points inside
    the image), first / last (the first and last inside k as Python ints, None where count is 0), nx / ny (points of the k walked
    whose x / y alone is inside: over all k when enumerated, over the window otherwise)."""
    res = int(resolution) or 512
    L = _beam_lines(buf, res, float(bounds_size))
    hi_px = float(res - 1)
    out = []
    for i in range(len(L["n"])):
        ax, ay, dx, dy, n = (float(L[f][i]) for f in ("ax", "ay", "dx", "dy", "n"))
        row = dict(n=n if np.isfinite(n) else None, drawn=bool(L["ok"][i]), windowed=False, count=0, first=None, last=None, nx=0, ny=0)
        out.append(row)
        if not row["drawn"]:
            continue
        row["windowed"] = _windowed(dx, dy, n, beam_route)
        lo, hi = _window(ax, ay, dx, dy, n, res) if row["windowed"] else (0, int(n))
        assert hi - lo + 1 <= max_work, "beam_spans: too many beam points"
        for k in _k_chunks(lo, hi):
            px = np.floor(ax + dx * k / n)
            py = np.floor(ay + dy * k / n)
            inx = (px >= 0) & (px <= hi_px)
            iny = (py >= 0) & (py <= hi_px)
            ins = np.nonzero(inx & iny)[0]
            row["nx"] += int(inx.sum())
            row["ny"] += int(iny.sum())
            if len(ins):
                row["count"] += len(ins)
                if row["first"] is None:
                    row["first"] = int(k[ins[0]])
                row["last"] = int(k[ins[-1]])
    return out


def render_ref(buf, resolution=512, bounds_size=1000.0, particle_radius=10.0, max_work=400_000_000, beam_route=None):
    assert beam_route in (None, "enumerate", "window")
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
        bx = particle_boxes(buf, res, S, r)
        cx, cy, ok, cx0, cx1, cy0, cy1 = (bx[f] for f in ("cx", "cy", "ok", "cx0", "cx1", "cy0", "cy1"))
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
        L = _beam_lines(buf, res, S)
        beam_cols = _beam_colours(L["rec"]["strain"], L["rec"]["stress"])
        ax, ay, dx, dy, n, ok = (L[f] for f in ("ax", "ay", "dx", "dy", "n", "ok"))
        win = np.zeros(B, dtype=bool)
        for i in np.nonzero(ok & ((n + 1 > WINDOW_THRESHOLD) | (beam_route == "window")))[0]:
            win[i] = _windowed(float(dx[i]), float(dy[i]), float(n[i]), beam_route)
        # the window route, a beam at a time
        for i in np.nonzero(win)[0]:
            lo, hi = _window(float(ax[i]), float(ay[i]), float(dx[i]), float(dy[i]), float(n[i]), res)
            assert hi - lo + 1 <= max_work, "render_ref: too many beam points"
            for k in _k_chunks(lo, hi):
                put(np.floor(ax[i] + dx[i] * k / n[i]), np.floor(ay[i] + dy[i] * k / n[i]), np.full(len(k), 2 * P + int(i), dtype=np.int64))
        # the enumerating route, many beams at a time
        sl = np.nonzero(ok & ~win)[0]
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
