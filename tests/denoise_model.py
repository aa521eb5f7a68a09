"""The denoiser's rule (include/raytrace_amd.h, "denoiser") restated in numpy f64 -- a helper of
test_denoise_model.py (which pins it against a plain scalar-loop restatement and states its properties on the
CPU) and of test_gpu_denoise.py (which holds the device to it, bit for bit).

Vectorised over the pixels, one tap at a time in the header's order (dy outer, dx inner): for the tap offset
o = s * (dx, dy) the pixels p whose tap p + o lies inside the image are a rectangle of the image, and their taps
the same rectangle shifted by o.  Every statement below is one numpy ufunc call on float64 arrays, an IEEE
operation with one rounding each, so the vectorised form computes what the scalar statements would.

denoise() returns its intermediates: the (demodulated) f32 input of every pass, the f64 result of the last pass
before and after remodulation, the f32 output and the BGR bytes.
"""
import numpy as np

import output_model as om

NORMAL, DEPTH, COLOR, DEMODULATE = 1, 2, 4, 8
ALL_MASKS = tuple(range(16))
K = (0.375, 0.25, 0.0625)          # 3/8, 1/4, 1/16
DEFAULTS = dict(iterations=5, flags=NORMAL | DEPTH, normal_squarings=5, sigma_color=1.0, sigma_depth=0.05)


def _f64(a):
    return None if a is None else np.asarray(a, np.float32).astype(np.float64)


def demodulate(rgb, albedo):
    """c = a > 0.0 ? (double)(float)(c / a) : c, per channel -> float32."""
    c, a = _f64(rgb), _f64(albedo)
    with np.errstate(all="ignore"):
        return np.where(a > 0.0, om.to_f32(c / a), np.asarray(rgb, np.float32)).astype(np.float32)


def filter_pass(c32, s, flags, normal=None, depth=None, normal_squarings=0, sigma_color=1.0, sigma_depth=1.0):
    """One pass of step s over the f32 colours c32 [h, w, 3] -> (v f64 [h, w, 3], wsum f64 [h, w], kept int [h, w]:
    the taps each pixel kept, its own included)."""
    c = _f64(c32)
    n, z = _f64(normal), _f64(depth)
    h, w, _ = c.shape
    total = np.zeros((h, w, 3), np.float64)
    wsum = np.zeros((h, w), np.float64)
    kept = np.zeros((h, w), np.int64)
    finite = np.isfinite(c).all(axis=2)
    with np.errstate(all="ignore"):
        t = np.float64(sigma_depth) * np.float64(s)
        tt = t * t
        sc = np.float64(sigma_color) / np.float64(s)
        scsc = sc * sc
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = s * dy, s * dx
                y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                kw = np.float64(K[abs(dy)]) * np.float64(K[abs(dx)])
                wt = np.full((y1 - y0, x1 - x0), kw, np.float64)
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
                    if flags & COLOR:
                        dc = c[P] - c[Q]
                        e = (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]
                        wt = wt / (1.0 + e / scsc)
                    keep = (wt > 0.0) & finite[Q]
                total[P] = np.where(keep[..., None], total[P] + wt[..., None] * c[Q], total[P])
                wsum[P] = np.where(keep, wsum[P] + wt, wsum[P])
                kept[P] += keep
        v = total / wsum[..., None]
    return v, wsum, kept


def denoise(rgb, normal=None, depth=None, albedo=None, iterations=5, flags=NORMAL | DEPTH, normal_squarings=5,
            sigma_color=1.0, sigma_depth=0.05, bgr_pitch=0):
    """The whole rule.  Returns {"inputs": [f32 image per pass], "kept": [per pass], "v_filtered": f64, "v": f64 (after
    remodulation), "rgb": f32, "bgr": uint8 [h, pitch]}."""
    assert 1 <= iterations <= 8
    cur = np.asarray(rgb, np.float32)
    if flags & DEMODULATE:
        cur = demodulate(cur, albedo)
    inputs, kepts = [], []
    v = None
    for i in range(iterations):
        inputs.append(cur)
        v, _, kept = filter_pass(cur, 1 << i, flags, normal, depth, normal_squarings, sigma_color, sigma_depth)
        kepts.append(kept)
        cur = om.to_f32(v)
    out = v
    if flags & DEMODULATE:
        a = _f64(albedo)
        with np.errstate(all="ignore"):
            out = np.where(a > 0.0, v * a, v)
    return {"inputs": inputs, "kept": kepts, "v_filtered": v, "v": out, "rgb": om.to_f32(out),
            "bgr": om.bgr_rows(out, bgr_pitch)}


# ---- the same rule as plain scalar loops (Python floats are IEEE f64) ------------------------------------
def scalar_pass(c32, s, flags, normal=None, depth=None, normal_squarings=0, sigma_color=1.0, sigma_depth=1.0):
    c = _f64(c32).tolist()
    n = None if normal is None else _f64(normal).tolist()
    z = None if depth is None else _f64(depth).tolist()
    h, w = len(c), len(c[0])
    inf = float("inf")
    out = np.zeros((h, w, 3), np.float64)

    def div(a, b):                     # IEEE division where Python raises
        if b == 0.0:
            if a != a or a == 0.0:
                return float("nan")
            neg = (np.copysign(1.0, a) < 0) != (np.copysign(1.0, b) < 0)
            return -inf if neg else inf
        return a / b

    for y in range(h):
        for x in range(w):
            sm = [0.0, 0.0, 0.0]
            ws = 0.0
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
                            wt = div(wt, 1.0 + div(dz * dz, t * t))
                        if flags & COLOR:
                            cp = c[y][x]
                            dr, dg, db = cp[0] - cq[0], cp[1] - cq[1], cp[2] - cq[2]
                            e = (dr * dr + dg * dg) + db * db
                            sc = div(sigma_color, float(s))
                            wt = div(wt, 1.0 + div(e, sc * sc))
                        if not (wt > 0.0 and all(abs(v) < inf for v in cq)):
                            continue
                    for k in range(3):
                        sm[k] = sm[k] + wt * cq[k]
                    ws = ws + wt
            for k in range(3):
                out[y, x, k] = div(sm[k], ws)
    return out


def scalar_denoise(rgb, normal=None, depth=None, albedo=None, iterations=5, flags=NORMAL | DEPTH, normal_squarings=5,
                   sigma_color=1.0, sigma_depth=0.05):
    """-> (v f64 after remodulation, rgb f32)."""
    cur = np.asarray(rgb, np.float32)
    if flags & DEMODULATE:
        cur = demodulate(cur, albedo)
    v = None
    for i in range(iterations):
        v = scalar_pass(cur, 1 << i, flags, normal, depth, normal_squarings, sigma_color, sigma_depth)
        cur = om.to_f32(v)
    if flags & DEMODULATE:
        a = _f64(albedo)
        with np.errstate(all="ignore"):
            v = np.where(a > 0.0, v * a, v)
    return v, om.to_f32(v)


# ---- images ----------------------------------------------------------------------------------------------
def random_image(h, w, seed, special=False):
    """Colours, unit-ish normals, depths and albedos of an h x w image; special: NaN and inf colours, NaN depths, zero
    normals (misses), zero albedo channels and -0.0 sprinkled in."""
    r = np.random.default_rng(seed)
    rgb = r.random((h, w, 3), np.float32) * np.float32(2.0)
    nrm = r.normal(size=(h, w, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(np.float32)
    nrm[:, : max(1, w // 2)] = nrm[0, 0]                     # a flat region: taps that pass the normal test
    depth = (4.0 + r.random((h, w)) * 0.5).astype(np.float32)
    albedo = (0.1 + 0.9 * r.random((h, w, 3))).astype(np.float32)
    if special:
        def some(k):
            return r.integers(0, h, k), r.integers(0, w, k)
        k = max(1, h * w // 12)
        rgb[some(k) + (r.integers(0, 3, k),)] = np.nan
        rgb[some(k) + (r.integers(0, 3, k),)] = np.inf
        rgb[some(k) + (r.integers(0, 3, k),)] = -np.inf
        rgb[some(k) + (r.integers(0, 3, k),)] = -0.0
        rgb[some(k)] = 0.0
        depth[some(k)] = np.nan
        nrm[some(k)] = 0.0
        albedo[some(k) + (r.integers(0, 3, k),)] = 0.0
        albedo[some(k) + (r.integers(0, 3, k),)] = -0.0
    return rgb, nrm, depth, albedo


def same_f32(a, b):
    """f32 arrays equal in every bit, non-finite values by position (a NaN's payload is left open)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(om.same_f32(a, b).all())
