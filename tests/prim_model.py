"""The record-level probes (include/raytrace_amd.h: rt_isect_check, rt_shade_check) restated in f64 numpy,
operation by operation -- a helper of test_prim_model.py (which pins it against the oracle's own building
blocks on the CPU) and of test_gpu_prims.py (which compares the device with it, bit for bit) -- and the
records both feed it: operand classes built to sit on each decision of the sphere test, the plane test and
the shading terms.

numpy's float64 +, -, *, / and sqrt are the IEEE operations, one rounding each, and every one below is a
ufunc call of its own: nothing is fused.  Dots are (x x' + y y') + z z' (nalgebra's order, as oracle/ref64.c
and aov_model.py assume it).  The only function that is not an IEEE operation is pow: np.power is numpy's
own, within one representable value of the C library's that the oracle calls (test_prim_model.py), so
shade() takes the powers from its caller wherever bits matter.
"""
import numpy as np

K_MIN_SIGNIFICANCE = 1.0 / 256.0 / 2.0          # raytrace.rs:17
K_EPS = 0.00001                                 # raytrace.rs:43,62
K_FRAC_1_PI = 0.318309886183790671537767526745028724
MAT_PHONG, MAT_FRESNEL = 0, 2                   # rt_material_kind
LIGHT_POINT, LIGHT_DIRECTIONAL = 0, 1           # rt_light_kind
TWO_PI = 2.0 * 3.14159265358979323846264338327950288     # the path kernel's 2.0 * kPi


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def bits_equal(p, q):
    """Bitwise equality, NaN == NaN (payloads aside)."""
    p, q = np.ascontiguousarray(p, np.float64), np.ascontiguousarray(q, np.float64)
    return (p.view(np.uint64) == q.view(np.uint64)) | (np.isnan(p) & np.isnan(q))


def biased_exponent(x):
    return ((np.ascontiguousarray(x, np.float64).view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)


def ordinal(x):
    """float64 -> int64, monotone over the finite values and the infinities: the distance between two
    values in representable values is the difference of their ordinals (+0 and -0 are the same value)."""
    b = np.ascontiguousarray(x, np.float64).view(np.int64)
    return np.where(b < 0, np.int64(-2 ** 63) - b, b)


def low16_distance(x, low16):
    """The signed distance, in representable values, of x from the values whose ordinals' low 16 bits are
    `low16` (tests/golden/libm_cr.npz), right when it is below 2^15: the caller bounds x first."""
    return ((ordinal(x) - low16.astype(np.int64) + 32768) & 0xFFFF) - 32768


def clamp_zero(x):
    return np.where(x < 0.0, 0.0, x)            # raytrace.rs:20-23: NaN and -0 pass through


# ---- shapes.rs:50-112 ---------------------------------------------------------------------------------
def sphere(o, d, c, radius):
    """Sphere::intersect for records (o, d, c [n, 3], radius [n]): hit, t, the hit point ray.cast(t), the
    normal, and the intermediates the coverage conditions read.  A miss has t 0 and a zero point and normal,
    as the probe reports it."""
    with np.errstate(all="ignore"):
        oc = o - c
        a = dot(d, d)
        b = 2.0 * dot(d, oc)
        cc = dot(oc, oc) - radius * radius
        disc = b * b - (4.0 * a) * cc
        pos = disc > 0.0
        s = np.sqrt(disc)
        a2 = 2.0 * a
        x1, x2 = -b - s, -b + s
        t1, t2 = x1 / a2, x2 / a2
        first = pos & (t1 > 0.0)
        second = pos & ~first & (t2 > 0.0)
        hit = first | second
        t = np.where(first, t1, np.where(second, t2, 0.0))
        pt = o + d * t[:, None]
        u = pt - c
        nrm = u / np.sqrt(dot(u, u))[:, None]
    z = ~hit
    pt[z] = 0.0
    nrm[z] = 0.0
    return {"hit": hit, "t": t, "pt": pt, "n": nrm, "disc": disc, "a2": a2, "x1": x1, "x2": x2, "second": second}


def plane(o, d, p, n):
    """Plane::intersect: t as computed and the verdict `not t <= 0` (a NaN t is a hit)."""
    with np.errstate(all="ignore"):
        num, den = dot(n, p - o), dot(n, d)
        t = num / den
        return {"hit": ~(t <= 0.0), "t": t, "num": num, "den": den}


# ---- raytrace.rs:30-62, 123-163; scene.rs:122-138 ------------------------------------------------------
def light_dir(kind, lv, pt):
    with np.errstate(all="ignore"):
        v = lv - pt
        r2 = dot(v, v)
        point = kind == LIGHT_POINT
        ldir = np.where(point[:, None], v / np.sqrt(r2)[:, None], -lv)
        return ldir, np.where(point, r2, 0.0), point


def fresnel_factor(ior, nd):
    with np.errstate(all="ignore"):
        r0 = (ior - 1.0) / (ior + 1.0)
        r0 = r0 * r0
        omcos = 1.0 - np.abs(nd)
        omcos2 = omcos * omcos
        f = r0 + (((1.0 - r0) * omcos2) * omcos2) * omcos
        return np.where(f > 1.0, 1.0, f)


def add_light(res, kd, ks, lc, f, ldir, n, p, diffuse, specular):
    """The colour after one unshadowed light: res + ((kd lc) s) 1/pi where `diffuse`, then + ((ks lc) f) p
    where `specular` (f = 1 for Phong: x * 1.0 is x)."""
    with np.errstate(all="ignore"):
        s = clamp_zero(dot(ldir, n))
        res = np.where(diffuse[:, None], res + ((kd * lc) * s[:, None]) * K_FRAC_1_PI, res)
        return np.where(specular[:, None], res + ((ks * lc) * f[:, None]) * p[:, None], res)


def shade(pt, rn, d, kd, ks, exponent, ior, mat, lkind, lv, lc, sig, p=None):
    """Every output of rt_shade_check but the three libm columns.  p: the powers to fold into the colour
    instead of np.power's (the device's own, when the device's colour is checked)."""
    with np.errstate(all="ignore"):
        nd = dot(rn, d)
        n = np.where((nd > 0.0)[:, None], -rn, rn)
        ldir, r2, has_range = light_dir(lkind, lv, pt)
        fres = fresnel_factor(ior, nd)
        f = np.where(mat == MAT_FRESNEL, fres, 1.0)
        kd_sig, ks_sig = (kd[:, 0] + kd[:, 1]) + kd[:, 2], (ks[:, 0] + ks[:, 1]) + ks[:, 2]
        diffuse = kd_sig * sig > K_MIN_SIGNIFICANCE
        specular = (ks_sig * f) * sig > K_MIN_SIGNIFICANCE
        k2 = 2.0 * dot(d, n)
        rd = d - n * k2[:, None]
        refl = np.concatenate([pt + rd * K_EPS, rd], axis=1)
        h = ldir - d
        c = clamp_zero(dot(n, h / np.sqrt(dot(h, h))[:, None]))
        if p is None:
            p = np.power(c, exponent)
        on = np.ones(len(c), bool)
        col = add_light(np.zeros_like(pt), kd, ks, lc, f, ldir, n, p, on, on)
    return {"ldir": ldir, "r2": r2, "has_range": has_range, "fresnel": fres, "f": f, "diffuse": diffuse,
            "specular": specular, "refl": refl, "c": c, "p": p, "col": col, "n": n, "nd": nd}


# ---- records --------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.sqrt(dot(v, v))[:, None]


def _perp(rng, d):
    v = np.cross(d, _unit(rng, len(d)))
    return v / np.sqrt(dot(v, v))[:, None]


def _operating(rng, n):
    """Unit directions, radii 0.01-10, coordinates within +-50, rays aimed inside 1.3 radii of the centre."""
    c = rng.uniform(-50.0, 50.0, (n, 3))
    radius = 10.0 ** rng.uniform(-2.0, 1.0, n)
    o = rng.uniform(-50.0, 50.0, (n, 3))
    aim = c + _unit(rng, n) * (radius * 1.3 * rng.uniform(0.0, 1.0, n) ** 2)[:, None]
    d = aim - o
    return o, d / np.sqrt(dot(d, d))[:, None], c, radius


SPECIALS = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, 1e-150, -1e-150, 1e150, -1e150, np.inf, -np.inf, np.nan, 1.0])
PLANE_SPECIALS = ("nan_0_0", "pos_inf", "neg_inf", "pos_zero", "neg_zero", "len_1e-35", "len_1e34", "inf_minus_inf")
SCALES = (-540, -512, -500, -400, -250, -100, 100, 250, 400, 500, 512, 540)
A2_EXPONENTS = tuple(range(920, 927)) + tuple(range(1120, 1127))


def isect_records(seed=20261020, unit=1 << 14):
    """(rays [n, 6], spheres [n, 4], planes [n, 6], labels [n] of str) with n = 106.5 * unit (1,744,896 at the default): the classes of
    the sphere and plane tests, each on one of their decisions."""
    rng = np.random.default_rng(seed)
    O, D, C, R, P, N, lab = [], [], [], [], [], [], []

    def emit(name, o, d, c, r, p=None, nv=None):
        n = len(r)
        if p is None:                      # an ordinary plane: the sphere classes' rays meet it anywhere
            p = rng.uniform(-50.0, 50.0, (n, 3))
            nv = _unit(rng, n) * (10.0 ** rng.uniform(-2.0, 2.0, n))[:, None]
        for lst, v in zip((O, D, C, R, P, N), (o, d, c, r, p, nv)):
            lst.append(np.array(v, np.float64))
        lab.append(np.full(n, name))

    # 1. the renders' operating point
    emit("operating", *_operating(rng, 32 * unit))
    # 2a. grazing, exactly: small-integer lattices (every product and sum exact, disc == 0 reachable)
    n = 16 * unit
    emit("lattice", rng.integers(-8, 9, (n, 3)), rng.integers(-4, 5, (n, 3)), rng.integers(-8, 9, (n, 3)),
         rng.integers(0, 9, n))
    # 2b. grazing, nearly: the sphere moved onto the ray's tangent, its radius nudged by +-1..3 values
    n = 8 * unit
    o, d, c, r = _operating(rng, n)
    c = (o + d * rng.uniform(1.0, 60.0, n)[:, None]) + _perp(rng, d) * r[:, None]
    k = rng.integers(1, 4, n) * rng.choice([-1, 1], n)
    emit("tangent", o, d, c, (ordinal(r) + k).view(np.float64))
    # 3. origins on the surface (the shadow and mirror rays start there), moved +-1e-5 along the direction,
    #    inside the sphere, in front of a sphere that lies behind, and zero radii
    n = 4 * unit
    for name, off in (("surface", 0.0), ("surface+eps", K_EPS), ("surface-eps", -K_EPS)):
        _, d, c, r = _operating(rng, n)
        emit(name, (c + _unit(rng, n) * r[:, None]) + d * off, d, c, r)
    n = 2 * unit
    _, d, c, r = _operating(rng, n)
    emit("inside", c + _unit(rng, n) * (r * rng.uniform(0.0, 0.999, n))[:, None], d, c, r)
    _, d, c, r = _operating(rng, n)
    emit("behind", c + d * (r * rng.uniform(1.01, 5.0, n))[:, None], d, c, r)
    o, d, c, r = _operating(rng, n)
    emit("zero_radius", o, d, c, np.zeros(n))
    # 4. direction lengths that put the biased exponent of 2a on both sides of both edges of div_k's window
    n = unit
    for e in A2_EXPONENTS:
        o, d, c, r = _operating(rng, n)
        a2 = ((np.uint64(e) << np.uint64(52)) | rng.integers(0, 1 << 52, n, dtype=np.uint64)).view(np.float64)
        emit(f"a2_{e}", o, d * np.sqrt(a2 / 2.0)[:, None], c, r)
    #    ... and far outside it, where the reciprocal of 2a leaves the normal numbers and only the real division
    #    answers (just outside the window the three correction operations still round correctly): 2a in
    #    [2^-1030, 2^-1020], and 2a in [2^1019, 2^1023] on geometry 2^-9 the size so that b b stays finite
    o, d, c, r = _operating(rng, n)
    emit("a2_tiny", o, d * np.sqrt(2.0 ** rng.uniform(-1030.0, -1020.0, n) / 2.0)[:, None], c, r)
    o, d, c, r = _operating(rng, n)
    emit("a2_huge", o * 2.0 ** -9, d * np.sqrt(2.0 ** rng.uniform(1019.0, 1023.0, n) / 2.0)[:, None], c * 2.0 ** -9, r * 2.0 ** -9)
    # 5. the whole configuration scaled by 2^k
    for k in SCALES:
        o, d, c, r = _operating(rng, n)
        s = 2.0 ** k
        emit(f"scale_{k}", o * s, d, c * s, r * s)
    # 6. specials in origin, direction, centre and radius; zero directions
    n = 4 * unit
    o, d, c, r = _operating(rng, n)
    rec = np.concatenate([o, d, c, r[:, None]], axis=1)
    put = rng.uniform(0.0, 1.0, rec.shape) < 0.25
    rec[put] = rng.choice(SPECIALS, int(put.sum()))
    rec[: n // 8, 3:6] = rng.choice(np.array([0.0, -0.0]), (n // 8, 3))
    emit("specials", rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9])
    # 7. planes: each special of t = n.(p - o) / n.d on axis-aligned operands whose products are exact
    n = unit // 16
    for name in PLANE_SPECIALS:
        o, d, c, r = _operating(rng, n)
        p = rng.uniform(-50.0, 50.0, (n, 3))
        nv = _unit(rng, n)
        sgn = rng.choice([-1.0, 1.0], n)
        if name in ("nan_0_0", "pos_inf", "neg_inf"):          # n = (0, 0, nz), d = (dx, dy, 0): n.d = +-0
            nv = np.stack([np.zeros(n), np.zeros(n), sgn * rng.uniform(0.5, 2.0, n)], axis=1)
            # (0 dx + 0 dy) + nz 0 with dx, dy >= 0 is +0 whatever nz's sign: the quotient has the numerator's sign
            d = np.stack([np.abs(d[:, 0]), np.abs(d[:, 1]), np.zeros(n)], axis=1)
            gap = {"nan_0_0": 0.0, "pos_inf": 1.0, "neg_inf": -1.0}[name] * rng.uniform(0.5, 9.0, n)
            p[:, 2] = o[:, 2] + gap * sgn                      # numerator nz (pz - oz): 0, > 0, < 0
        elif name in ("pos_zero", "neg_zero"):                 # p = o: n.(p - o) = +0, n.d of either sign
            p = o.copy()
            want_neg = name == "neg_zero"
            den = dot(nv, d)
            nv = np.where(((den < 0.0) == want_neg)[:, None], nv, -nv)
        elif name == "len_1e-35":
            nv = nv * 1e-35
        elif name == "len_1e34":
            nv = nv * 1e34
        else:                                                  # products overflow to inf - inf
            nv = np.stack([np.full(n, 1e200), np.full(n, -1e200), nv[:, 2]], axis=1)
            p = o + np.stack([np.full(n, 1e200), np.full(n, 1e200), np.zeros(n)], axis=1)
        emit("plane_" + name, o, d, c, r, p, nv)
    cat = np.concatenate
    return cat([cat(O), cat(D)], axis=1), cat([cat(C), cat(R)[:, None]], axis=1), cat([cat(P), cat(N)], axis=1), cat(lab)


def coverage(rays, sph, pl, lab):
    """The conditions on the records that make the device comparison mean something, from the model's own
    intermediates (test_gpu_prims.py asserts them on the records it sends): counts by name."""
    m = sphere(rays[:, :3], rays[:, 3:], sph[:, :3], sph[:, 3])
    p = plane(rays[:, :3], rays[:, 3:], pl[:, :3], pl[:, 3:])
    e2 = biased_exponent(m["a2"])
    win = (e2 >= 923) & (e2 <= 1123)                 # div_k's window of 2a; outside it no numerator is in window

    def out_of_window(x):
        ex = biased_exponent(x)
        return (x > 0.0) & ~(win & (ex >= 123) & (ex <= 1622))
    pos = m["disc"] > 0.0
    sel = {s: lab == "plane_" + s for s in PLANE_SPECIALS}
    with np.errstate(all="ignore"):
        nlen = np.sqrt(dot(pl[:, 3:], pl[:, 3:]))
        fin = np.isfinite(pl).all(axis=1) & np.isfinite(rays).all(axis=1)
        cov = {"hits": m["hit"].sum(), "misses": (~m["hit"]).sum(), "second_root": m["second"].sum(),
               "disc_zero": (m["disc"] == 0.0).sum(), "disc_zero_lattice": ((m["disc"] == 0.0) & (lab == "lattice")).sum(),
               "a2_below_window": ((e2 >= 920) & (e2 <= 922)).sum(), "a2_low_inside": ((e2 >= 923) & (e2 <= 926)).sum(),
               "a2_high_inside": ((e2 >= 1120) & (e2 <= 1123)).sum(), "a2_above_window": ((e2 >= 1124) & (e2 <= 1126)).sum(),
               "numerator_out_of_window": (pos & (out_of_window(m["x1"]) | out_of_window(m["x2"]))).sum(),
               "hits_2a_tiny": (m["hit"] & np.isfinite(m["t"]) & (lab == "a2_tiny")).sum(),
               "hits_2a_huge": (m["hit"] & (m["t"] > 0.0) & (lab == "a2_huge")).sum(),
               "plane_nan_0_0": (sel["nan_0_0"] & (p["num"] == 0.0) & (p["den"] == 0.0) & np.isnan(p["t"])).sum(),
               "plane_pos_inf": (sel["pos_inf"] & (p["den"] == 0.0) & (p["t"] == np.inf)).sum(),
               "plane_neg_inf": (sel["neg_inf"] & (p["den"] == 0.0) & (p["t"] == -np.inf)).sum(),
               "plane_pos_zero": (sel["pos_zero"] & (p["t"] == 0.0) & ~np.signbit(p["t"])).sum(),
               "plane_neg_zero": (sel["neg_zero"] & (p["t"] == 0.0) & np.signbit(p["t"])).sum(),
               "plane_len_1e-35": (sel["len_1e-35"] & (nlen < 2e-35) & (nlen > 5e-36)).sum(),
               "plane_len_1e34": (sel["len_1e34"] & (nlen < 2e34) & (nlen > 5e33)).sum(),
               "plane_inf_minus_inf": (sel["inf_minus_inf"] & fin & np.isnan(p["num"])).sum()}
    return {k: int(v) for k, v in cov.items()}, m, p


COVERAGE_FLOOR = {"hits": 10 ** 4, "misses": 10 ** 4, "second_root": 10 ** 4, "disc_zero": 500, "disc_zero_lattice": 500,
                  "a2_below_window": 10 ** 3, "a2_low_inside": 10 ** 3, "a2_high_inside": 10 ** 3, "a2_above_window": 10 ** 3,
                  "numerator_out_of_window": 10 ** 3, "hits_2a_tiny": 10 ** 3, "hits_2a_huge": 10 ** 3, **{"plane_" + s: 100 for s in PLANE_SPECIALS}}


EXPONENTS = np.array([0.0, 1.0, 2.0, 8.0, 32.0, 50.0, 1000.0, 0.5, 2.5, 1e-3])
IORS = np.array([1.0, 1.5, 1e-3, 1e3])


def shade_records(seed=20261021, n=1 << 19):
    """(records [m, 27] with the three libm columns zero, kinds [m, 2], labels [m]) with m = 2 n: the classes
    of the shading terms."""
    rng = np.random.default_rng(seed)
    out, kinds, lab = [], [], []

    def emit(name, m, rn=None, d=None, lkind=None, lv=None, sig=None, kd=None, pt=None):
        pt = rng.uniform(-50.0, 50.0, (m, 3)) if pt is None else pt
        rn = _unit(rng, m) if rn is None else rn
        d = _unit(rng, m) if d is None else d
        kd = rng.uniform(0.0, 1.0, (m, 3)) * (rng.uniform(0.0, 1.0, (m, 1)) < 0.9) if kd is None else kd
        ks = rng.uniform(0.0, 1.0, (m, 3)) * (rng.uniform(0.0, 1.0, (m, 1)) < 0.9)
        lkind = rng.integers(0, 2, m) if lkind is None else lkind
        if lv is None:                     # point lights 1e-3 .. 1e6 away, directional ones 1e-35 .. 1e34 long
            far = pt + _unit(rng, m) * (10.0 ** rng.uniform(-3.0, 6.0, m))[:, None]
            lv = np.where((lkind == LIGHT_POINT)[:, None], far, _unit(rng, m) * (10.0 ** rng.uniform(-35.0, 34.0, m))[:, None])
        sig = 10.0 ** rng.uniform(-4.0, 0.0, m) if sig is None else sig
        rec = np.concatenate([pt, rn, d, kd, ks, rng.choice(EXPONENTS, m)[:, None],
                              np.where(rng.uniform(0, 1, m) < 0.5, rng.choice(IORS, m), rng.uniform(1.0, 3.0, m))[:, None],
                              lv, rng.uniform(0.0, 2.0, (m, 3)), sig[:, None], np.zeros((m, 3))], axis=1)
        out.append(rec)
        kinds.append(np.stack([rng.choice([MAT_PHONG, MAT_FRESNEL], m), lkind], axis=1).astype(np.int32))
        lab.append(np.full(m, name))

    emit("generic", n)
    q = n // 8
    # the light direction equal to the ray direction: a zero half vector, 0/0
    d = _unit(rng, q)
    emit("zero_half", q, d=d, lkind=np.full(q, LIGHT_DIRECTIONAL), lv=-d)
    # n.d = 0, +-1 on the axes; n = d and n = -d (|n.d| one value either side of 1); |n.d| above 1
    ax = np.eye(3)[rng.integers(0, 3, q)] * rng.choice([-1.0, 1.0], q)[:, None]
    emit("nd_zero", q, rn=ax, d=np.roll(ax, 1, axis=1))
    emit("nd_one", q, rn=ax, d=ax * rng.choice([-1.0, 1.0], q)[:, None])
    d = _unit(rng, q)
    emit("nd_near_one", q, rn=d * rng.choice([-1.0, 1.0], q)[:, None], d=d)
    emit("nd_above_one", q, rn=d * (rng.choice([-1.0, 1.0], q) * (1.0 + 10.0 ** rng.uniform(-15.0, -1.0, q)))[:, None], d=d)
    # significances on both sides of kMinSignificance and equal to it: kd sums to 1 exactly
    kd = np.tile(np.array([0.25, 0.25, 0.5]), (q, 1))
    k = rng.integers(-2, 3, q)
    emit("sig_edge", q, sig=(ordinal(np.full(q, K_MIN_SIGNIFICANCE)) + k).view(np.float64), kd=kd)
    emit("sig_wide", q, sig=K_MIN_SIGNIFICANCE * 2.0 ** rng.integers(-3, 4, q).astype(np.float64))
    # a light at the hit point itself: a zero light vector, 0/0
    pt = rng.uniform(-50.0, 50.0, (q, 3))
    emit("light_at_point", q, lkind=np.full(q, LIGHT_POINT), lv=pt, pt=pt)
    return np.concatenate(out), np.concatenate(kinds), np.concatenate(lab)


# ---- the libm operands (pow, sin, cos) ---------------------------------------------------------------------
POW_SPECIAL_X = np.array([0.0, -0.0, 1.0, np.nan, np.inf])
POW_SPECIAL_Y = np.array([0.0, -0.0, 1.0, np.nan, np.inf, -1.0])
N_FIXTURE = 20000


def _mix(z):
    """splitmix64's finaliser on uint64 arrays: the operands below are a pure function of their index, so
    the fixture's maker and its readers form the same ones without storing them."""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _u01(n, salt):
    """n values k 2^-53 of [0, 1)."""
    start = np.uint64((salt * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        z = _mix(np.arange(n, dtype=np.uint64) + start)
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def pow_operands(n, salt=1, normal_results=True):
    """(c, y): c over [0, 1 + 2^-50], every exponent of EXPONENTS in turn with each of four classes in turn:
    c uniform, dense near 0 (2^-60 and up), dense just below 1 (1 - u 2^-k, k = 1 .. 52) and just above it
    (1 + j 2^-52, j = 0 .. 4).  The class index (i // 10) % 4 shares no factor with the exponent index i % 10.
    normal_results (the correctly rounded fixture, whose maker rounds once to 53 bits): a c whose power
    would be subnormal or 0, c < lo = 2^-floor(1020 / y), is moved to the bottom of what is left -- the uniform
    class spreads over [lo, 1), the near-0 class sits within a factor 2 above lo, where y log c is largest -- so
    50 and 1000 keep uniform and small c wherever the result is a normal number (c >= 2^-20 and c >= 0.5).
    Without it nothing is moved: powers underflow through the subnormals to 0.  Every step is an IEEE
    operation or an exact scaling (ldexp), so every machine forms the same operands."""
    i = np.arange(n)
    u, v = _u01(n, salt), _u01(n, salt + 100)
    y = EXPONENTS[i % len(EXPONENTS)]
    cls = (i // len(EXPONENTS)) % 4
    uniform, near0 = u, np.ldexp(u, -np.floor(v * 60.0).astype(np.int64))
    if normal_results:
        lo = np.where(y > 1.0, np.ldexp(1.0, -np.floor(1020.0 / np.maximum(y, 1.0)).astype(np.int64)), 0.0)
        uniform = lo + (1.0 - lo) * u
        near0 = np.where(near0 < lo, lo * (1.0 + u), near0)
    below1 = 1.0 - np.ldexp(u, -np.floor(1.0 + v * 52.0).astype(np.int64))
    above1 = 1.0 + np.floor(u * 5.0) * 2.0 ** -52
    return np.select([cls == 0, cls == 1, cls == 2], [uniform, near0, below1], above1), y


def trig_operands(n, salt=2):
    """x = u 2 pi for u = k 2^-53 of [0, 1), the only arguments the path kernel forms; the last 24 are the u
    nearest m / 8 (x nearest the multiples of pi / 4, pi / 2 among them) and their two neighbours."""
    u = _u01(n, salt)
    m = np.repeat(np.arange(8, dtype=np.float64) / 8.0, 3) + np.tile(np.array([-1.0, 0.0, 1.0]) * 2.0 ** -53, 8)
    u[n - 24:] = np.where(m < 0.0, 1.0 - 2.0 ** -53, m)
    return u * TWO_PI
