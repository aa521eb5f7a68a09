"""The variance-guided denoiser's rule (include/raytrace_amd.h, "denoiser, variance-guided") restated in numpy f64 -- a
helper of test_denoise_var_model.py (which pins it against a plain scalar-loop restatement and states its properties
on the CPU) and of test_gpu_denoise_var.py (which holds the device to it, bit for bit).

Everything denoise_model.py says of itself holds here: one tap at a time in the header's order, every statement one
numpy ufunc call on float64 arrays, so one IEEE operation with one rounding each.  What the rule adds to rt_denoise's
is marked "(added)".

denoise_var() returns its intermediates: per pass the f32 input colours, the f32 input variance, the prefiltered
variance g and the taps kept; the f64 colours of the last pass before and after remodulation, the f64 variance x of
the last pass, the f32 outputs and the BGR bytes.
"""
import numpy as np

import denoise_model as dm
import output_model as om

from denoise_model import ALL_MASKS, COLOR, DEMODULATE, DEPTH, NORMAL, K   # noqa: F401  (the same flags and kernel)

G = (0.5, 0.25)                    # 1/2, 1/4: the 3 x 3 prefilter of the variance
VAR_DEFAULTS = dict(sigma_variance=2.0, variance_floor=2.0 ** -20)

_f64 = dm._f64


def pack_variance(variance, flags, albedo=None):
    """(added) [h, w, 3] f32 per-channel variances -> [h, w] f32: the record's fourth float."""
    u = _f64(variance)
    with np.errstate(all="ignore"):
        if flags & DEMODULATE:
            a = _f64(albedo)
            u = np.where(a > 0.0, u / (a * a), u)
        u = np.where(u > 0.0, u, 0.0)
        return om.to_f32((u[..., 0] + u[..., 1]) + u[..., 2])


def _rects(h, w, oy, ox):
    """The pixels p whose neighbour p + (ox, oy) lies inside the image, and those neighbours: (P, Q) or None."""
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def prefilter(var32):
    """(added) g = gs / gw over the 3 x 3 pixels around each pixel, always one pixel apart -> f64 [h, w]."""
    var = _f64(var32)
    h, w = var.shape
    gs = np.zeros((h, w), np.float64)
    gw = np.zeros((h, w), np.float64)
    with np.errstate(all="ignore"):
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                r = _rects(h, w, dy, dx)
                if r is None:
                    continue
                P, Q = r
                gk = np.float64(G[abs(dy)]) * np.float64(G[abs(dx)])
                gs[P] = gs[P] + gk * var[Q]
                gw[P] = gw[P] + gk
        return gs / gw


def filter_pass(c32, var32, s, flags, normal=None, depth=None, normal_squarings=0, sigma_color=1.0, sigma_depth=1.0,
                sigma_variance=2.0, variance_floor=2.0 ** -20):
    """One pass of step s over the f32 colours c32 [h, w, 3] and variances var32 [h, w] -> (v f64 [h, w, 3], x f64
    [h, w], g f64 [h, w], wsum f64 [h, w], kept int [h, w])."""
    c, var = _f64(c32), _f64(var32)
    n, z = _f64(normal), _f64(depth)
    h, w, _ = c.shape
    total = np.zeros((h, w, 3), np.float64)
    wsum = np.zeros((h, w), np.float64)
    vs = np.zeros((h, w), np.float64)
    kept = np.zeros((h, w), np.int64)
    finite = np.isfinite(c).all(axis=2)
    g = prefilter(var32)
    with np.errstate(all="ignore"):
        den = (np.float64(sigma_variance) * np.float64(sigma_variance)) * g + np.float64(variance_floor)     # (added)
        t = np.float64(sigma_depth) * np.float64(s)
        tt = t * t
        sc = np.float64(sigma_color) / np.float64(s)
        scsc = sc * sc
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                r = _rects(h, w, s * dy, s * dx)
                if r is None:
                    continue
                P, Q = r
                kw = np.float64(K[abs(dy)]) * np.float64(K[abs(dx)])
                wt = np.full(wsum[P].shape, kw, np.float64)
                if dy == 0 and dx == 0:
                    keep = np.ones(wt.shape, bool)
                else:
                    if flags & NORMAL:
                        d = (n[P][..., 0] * n[Q][..., 0] + n[P][..., 1] * n[Q][..., 1]) + n[P][..., 2] * n[Q][..., 2]
                        d = np.where(d > 0.0, d, 0.0)
                        for _ in range(normal_squarings):
                            d = d * d
                        wt = wt * d
                    if flags & DEPTH:
                        dz = z[P] - z[Q]
                        wt = wt / (1.0 + (dz * dz) / tt)
                    dc = c[P] - c[Q]
                    e = (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]
                    if flags & COLOR:
                        wt = wt / (1.0 + e / scsc)
                    wt = wt / (1.0 + e / den[P])                                                            # (added)
                    keep = (wt > 0.0) & finite[Q]
                total[P] = np.where(keep[..., None], total[P] + wt[..., None] * c[Q], total[P])
                wsum[P] = np.where(keep, wsum[P] + wt, wsum[P])
                vs[P] = np.where(keep, vs[P] + (wt * wt) * var[Q], vs[P])                                   # (added)
                kept[P] += keep
        v = total / wsum[..., None]
        x = vs / (wsum * wsum)                                                                              # (added)
        x = np.where(x > 0.0, x, 0.0)
    return v, x, g, wsum, kept


def denoise_var(rgb, variance, normal=None, depth=None, albedo=None, iterations=5, flags=NORMAL | DEPTH, normal_squarings=5,
                sigma_color=1.0, sigma_depth=0.05, bgr_pitch=0, sigma_variance=2.0, variance_floor=2.0 ** -20):
    """The whole rule.  Returns {"inputs": [f32 colours per pass], "variances": [f32 variance per pass], "g": [per pass],
    "kept": [per pass], "v_filtered": f64, "v": f64 (after remodulation), "x": f64 [h, w], "rgb": f32, "bgr": uint8
    [h, pitch], "variance": f32 [h, w]}."""
    assert 1 <= iterations <= 8
    cur = np.asarray(rgb, np.float32)
    if flags & DEMODULATE:
        cur = dm.demodulate(cur, albedo)
    var = pack_variance(variance, flags, albedo)
    inputs, variances, gs, kepts = [], [], [], []
    v = x = None
    for i in range(iterations):
        inputs.append(cur)
        variances.append(var)
        v, x, g, _, kept = filter_pass(cur, var, 1 << i, flags, normal, depth, normal_squarings, sigma_color, sigma_depth,
                                       sigma_variance, variance_floor)
        gs.append(g)
        kepts.append(kept)
        cur, var = om.to_f32(v), om.to_f32(x)
    out = v
    if flags & DEMODULATE:
        a = _f64(albedo)
        with np.errstate(all="ignore"):
            out = np.where(a > 0.0, v * a, v)
    return {"inputs": inputs, "variances": variances, "g": gs, "kept": kepts, "v_filtered": v, "v": out, "x": x,
            "rgb": om.to_f32(out), "bgr": om.bgr_rows(out, bgr_pitch), "variance": om.to_f32(x)}


# ---- the same rule as plain scalar loops (Python floats are IEEE f64) ------------------------------------
def _div(a, b):                        # IEEE division where Python raises
    if b == 0.0:
        if a != a or a == 0.0:
            return float("nan")
        neg = (np.copysign(1.0, a) < 0) != (np.copysign(1.0, b) < 0)
        return float("-inf") if neg else float("inf")
    return a / b


def scalar_pack(variance, flags, albedo=None):
    u32 = np.asarray(variance, np.float32)
    h, w, _ = u32.shape
    a32 = None if albedo is None else np.asarray(albedo, np.float32)
    out = np.zeros((h, w), np.float64)
    for y in range(h):
        for x in range(w):
            u = [float(u32[y, x, k]) for k in range(3)]
            for k in range(3):
                if flags & DEMODULATE:
                    a = float(a32[y, x, k])
                    if a > 0.0:
                        u[k] = _div(u[k], a * a)
                u[k] = u[k] if u[k] > 0.0 else 0.0
            out[y, x] = (u[0] + u[1]) + u[2]
    return om.to_f32(out)


def scalar_pass(c32, var32, s, flags, normal=None, depth=None, normal_squarings=0, sigma_color=1.0, sigma_depth=1.0,
                sigma_variance=2.0, variance_floor=2.0 ** -20):
    """-> (v f64 [h, w, 3], x f64 [h, w])."""
    c = _f64(c32).tolist()
    var = _f64(var32).tolist()
    n = None if normal is None else _f64(normal).tolist()
    z = None if depth is None else _f64(depth).tolist()
    h, w = len(c), len(c[0])
    inf = float("inf")
    out = np.zeros((h, w, 3), np.float64)
    outx = np.zeros((h, w), np.float64)
    sigma_variance, variance_floor = float(sigma_variance), float(variance_floor)
    for y in range(h):
        for x in range(w):
            gs = gw = 0.0
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    qy, qx = y + dy, x + dx
                    if qy < 0 or qy >= h or qx < 0 or qx >= w:
                        continue
                    gk = G[abs(dy)] * G[abs(dx)]
                    gs = gs + gk * var[qy][qx]
                    gw = gw + gk
            g = _div(gs, gw)
            den = (sigma_variance * sigma_variance) * g + variance_floor
            sm = [0.0, 0.0, 0.0]
            ws = vs = 0.0
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = y + s * dy, x + s * dx
                    if qy < 0 or qy >= h or qx < 0 or qx >= w:
                        continue
                    wt = K[abs(dy)] * K[abs(dx)]
                    cq = c[qy][qx]
                    if dy != 0 or dx != 0:
                        if flags & NORMAL:
                            a, b = n[y][x], n[qy][qx]
                            d = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
                            d = d if d > 0.0 else 0.0
                            for _ in range(normal_squarings):
                                d = d * d
                            wt = wt * d
                        if flags & DEPTH:
                            dz = z[y][x] - z[qy][qx]
                            t = sigma_depth * float(s)
                            wt = _div(wt, 1.0 + _div(dz * dz, t * t))
                        cp = c[y][x]
                        dr, dg, db = cp[0] - cq[0], cp[1] - cq[1], cp[2] - cq[2]
                        e = (dr * dr + dg * dg) + db * db
                        if flags & COLOR:
                            sc = _div(sigma_color, float(s))
                            wt = _div(wt, 1.0 + _div(e, sc * sc))
                        wt = _div(wt, 1.0 + _div(e, den))
                        if not (wt > 0.0 and all(abs(v) < inf for v in cq)):
                            continue
                    for k in range(3):
                        sm[k] = sm[k] + wt * cq[k]
                    ws = ws + wt
                    vs = vs + (wt * wt) * var[qy][qx]
            for k in range(3):
                out[y, x, k] = _div(sm[k], ws)
            xv = _div(vs, ws * ws)
            outx[y, x] = xv if xv > 0.0 else 0.0
    return out, outx


def scalar_denoise_var(rgb, variance, normal=None, depth=None, albedo=None, iterations=5, flags=NORMAL | DEPTH,
                       normal_squarings=5, sigma_color=1.0, sigma_depth=0.05, sigma_variance=2.0, variance_floor=2.0 ** -20):
    """-> (v f64 after remodulation, rgb f32, x f64, variance f32)."""
    cur = np.asarray(rgb, np.float32)
    if flags & DEMODULATE:
        cur = dm.demodulate(cur, albedo)
    var = scalar_pack(variance, flags, albedo)
    v = x = None
    for i in range(iterations):
        v, x = scalar_pass(cur, var, 1 << i, flags, normal, depth, normal_squarings, sigma_color, sigma_depth, sigma_variance,
                           variance_floor)
        cur, var = om.to_f32(v), om.to_f32(x)
    if flags & DEMODULATE:
        a = _f64(albedo)
        with np.errstate(all="ignore"):
            v = np.where(a > 0.0, v * a, v)
    return v, om.to_f32(v), x, om.to_f32(x)


# ---- images ----------------------------------------------------------------------------------------------
SPECIAL_VARIANCES = (np.nan, -1.0, -0.0, 0.0, np.inf, 2.0 ** -149, 2.0 ** -130, 2.0 ** 100)


def random_variance(h, w, seed, special=False):
    """A variance image [h, w, 3] f32 of ordinary magnitude; special: NaN, -1, -0.0, 0, +inf, f32 denormals and 2^100
    sprinkled in."""
    r = np.random.default_rng(seed)
    var = (r.random((h, w, 3), np.float32) * np.float32(0.05)).astype(np.float32)
    if special:
        k = max(1, h * w // 10)
        for value in SPECIAL_VARIANCES:
            var[r.integers(0, h, k), r.integers(0, w, k), r.integers(0, 3, k)] = np.float32(value)
    return var


def synthetic(seed=1, h=64, w=96, sigma=0.3, samples=4):
    """The image the variance guidance was designed on: two flat colour halves and a darkened rectangle, all with one
    normal and depth (no guide edge anywhere); the left third noise-free, the rest with Gaussian noise of standard
    deviation sigma per channel and sample.  -> dict(truth, noisy (the mean of the samples), variance (of the mean, by
    moments_model.estimate's rule), normal, depth)."""
    import moments_model as mm
    r = np.random.default_rng(seed)
    truth = np.empty((h, w, 3), np.float64)
    truth[:, : w // 2] = (0.9, 0.8, 0.2)
    truth[:, w // 2:] = (0.1, 0.2, 0.9)
    truth[h // 4: 3 * h // 4, w // 3: 2 * w // 3] *= 0.5
    noise = r.normal(scale=sigma, size=(samples, h, w, 3))
    noise[:, :, : w // 3] = 0.0
    stack = truth[None] + noise
    S, Q = mm.accumulate(stack)
    est = mm.estimate(S, Q, samples, 1e-3, 1.0)
    normal = np.zeros((h, w, 3), np.float32)
    normal[..., 2] = 1.0
    return dict(truth=truth.astype(np.float32), noisy=om.to_f32(S / np.float64(samples)), variance=est["variance"], normal=normal,
                depth=np.full((h, w), 4.0, np.float32))
