"""The conservative f32 culling arithmetic of the tree walks on the device (rt_cull_check:
make_raybox, t_limit, box_hit, the whole-LDS walk's near / far form, the compact stack entries;
DESIGN.md §4 "BVH exactness" items 1-3 and 6, and the far-origin rule) against f64 on the host.

Must hit: a box built by the host's rule around a sphere is never culled for a ray whose f64
quadratic (shapes.rs:60-88, the reference's operation order) reports a hit, at the limit that hit
sets.  Must miss: a ray whose exact slab interval on the box inflated by 1e-3 (1 + extent) is empty
is culled, so the widening cannot grow unnoticed.  Parity of whole frames sees neither directly:
it pins the first only where a ray happens to graze a box face, and the second not at all."""
import numpy as np
import pytest

import libraytrace as lr
import far_scenes

pytestmark = pytest.mark.gpu

LENGTHS = np.array([1.0, 1e-35, 1e34, 3e-7, 5e6])
OFFSETS = np.array([0.0, 0.5, 0.999999, 1.0, 1.000001, 1.5, 3.0])
CODES = np.array([-131072, -32769, -32768, -1, 0, 1, 32767, 32768, 131071], np.int32)
TINY = np.array([0.0, -0.0, 1e-300, -1e-300, 1e-9, -1e-9, 1e-4])


def _down32(x):
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f)


def _up32(x):
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f)


def _boxes(c, r, pad):
    """The host's sphere box (host_bvh.cpp): [c +- (r + pad)] rounded outward to f32."""
    return np.concatenate([_down32(c - r[:, None] - pad), _up32(c + r[:, None] + pad)], axis=1)


def _half_boxes(b):
    """The binary16 node's box (half_nodes): every f32 bound rounded outward to a half."""
    with np.errstate(over="ignore"):
        h = b.astype(np.float16)
        lo, hi = h[:, :3], h[:, 3:]
        lo = np.where(lo.astype(np.float32) > b[:, :3], np.nextafter(lo, np.float16(-np.inf)), lo)
        hi = np.where(hi.astype(np.float32) < b[:, 3:], np.nextafter(hi, np.float16(np.inf)), hi)
    return np.concatenate([lo, hi], axis=1).astype(np.float32)


def _quadratic(o, d, c, r):
    """t of the reference's sphere test per record (inf: None), in its operation order."""
    oc = o - c
    a = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    b = 2.0 * (d[:, 0] * oc[:, 0] + d[:, 1] * oc[:, 1] + d[:, 2] * oc[:, 2])
    cc = (oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1] + oc[:, 2] * oc[:, 2]) - r * r
    disc = b * b - (4.0 * a) * cc
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.sqrt(np.where(disc > 0.0, disc, 0.0))
        t1 = (-b - s) / (2.0 * a)
        t2 = (-b + s) / (2.0 * a)
    t = np.where(t1 > 0.0, t1, t2)
    return np.where((disc > 0.0) & (t > 0.0), t, np.inf)


def _aimed(rng, E, n, bound_mul, axis_share=0.5, beyond=None):
    """n (ray, sphere) records of one scene of extent about E: radii from 1e-6 (1 + E) upward, rays
    that pass their sphere at OFFSETS radii from its centre, along random and along nearly
    axis-parallel directions (lateral components 0, -0, 1e-300, 1e-9, 1e-4) of LENGTHS, from
    origins up to bound_mul (1 + ext) away from the coordinate origin on every axis."""
    c = rng.uniform(-E, E, (n, 3))
    r = (1.0 + E) * 10 ** rng.uniform(-6, -1, n)
    ext = far_scenes.extent(c, r)
    a = rng.normal(size=(n, 3))
    a /= np.linalg.norm(a, axis=1)[:, None]
    ax = rng.random(n) < axis_share
    k = rng.integers(0, 3, n)
    para = TINY[rng.integers(0, len(TINY), (n, 3))]
    para[np.arange(n), k] = rng.choice([-1.0, 1.0], n)
    a = np.where(ax[:, None], para, a)
    u = np.cross(a, rng.normal(size=(n, 3)))
    u /= np.linalg.norm(u, axis=1)[:, None]
    aim_at = OFFSETS[rng.integers(0, len(OFFSETS), n)] * r
    if beyond is not None:                  # ... plus one of these multiples of 1e-3 (1 + ext)
        aim_at = aim_at + beyond[rng.integers(0, len(beyond), n)] * 1e-3 * (1.0 + ext)
    target = c + u * aim_at[:, None]
    B = bound_mul * (1.0 + ext)
    L = B * 10 ** rng.uniform(-6, 0.3, n)
    for _ in range(8):                      # bring the origin inside the bound
        o = target - a * L[:, None]
        L = np.where(np.max(np.abs(o), axis=1) > B, 0.5 * L, L)
    o = target - a * L[:, None]
    keep = np.max(np.abs(o), axis=1) <= B
    d = a * LENGTHS[rng.integers(0, len(LENGTHS), n)][:, None]
    return o[keep], d[keep], c[keep], r[keep], ext


def _exact_slab_empty(o, d, box, grow):
    """The slab interval of the ray on the box grown by `grow`, in f64 (the rounding of one
    subtraction and one division, 2e-16 relative, against a margin of 1e-3 (1 + extent)): True
    where it is empty or entirely behind the origin."""
    lo, hi = box[:, :3].astype(np.float64) - grow, box[:, 3:].astype(np.float64) + grow
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    inside = (lo <= o) & (o <= hi)
    zero = d == 0.0
    tmin = np.where(zero, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2))
    tmax = np.where(zero, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2))
    tn, tf = tmin.max(axis=1), tmax.min(axis=1)
    return (tn > tf) | (tf < 0.0)


def _check_must_hit(ctx, o, d, c, r, ext, reach, half=True):
    """Returns the number of records with a reported hit."""
    pad = far_scenes.PAD * (1.0 + ext)
    t = _quadratic(o, d, c, r)
    rays = np.concatenate([o, d], axis=1)
    codes = CODES[np.arange(len(t)) % len(CODES)]
    b32 = _boxes(c, r, pad)
    variants = [("f32", b32)] + ([("binary16", _half_boxes(b32))] if half and np.abs(b32).max() < 65504.0 else [])
    rep = np.isfinite(t)
    for name, box in variants:
        out = ctx.cull_check(rays, box, t, codes, reach)
        for form, hit, tn in (("box_hit", out["hit"], out["tnear"]), ("near/far", out["hit_nf"], out["tnear_nf"])):
            bad = rep & ~(hit & (tn <= out["tlim"]))
            assert not bad.any(), (f"{name} box, {form}: {bad.sum()} of {rep.sum()} reported hits culled, first: ray "
                                   f"{rays[bad][0].tolist()} sphere {c[bad][0].tolist()} r {r[bad][0]} t {t[bad][0]}")
        # the compact stack entries of (code, entry t): the code comes back, the t no larger and never NaN
        tn = out["tnear"]
        assert np.array_equal(out["node18"], codes)
        fits16 = (codes >= -32768) & (codes <= 32767)
        assert np.array_equal(out["node16"][fits16], codes[fits16])
        for tc in (out["t16"], out["t18"]):
            assert not (np.isnan(tc) & ~np.isnan(tn)).any()
            assert (tc[~np.isnan(tn)] <= np.maximum(tn[~np.isnan(tn)], 0.0)).all()
    return int(rep.sum())


@pytest.mark.parametrize("E", [1.0, 1e3, 1e6])
def test_reported_hits_are_never_culled(gpu_ctx, E):
    """Origins within 10 (1 + ext) and, a second set, up to the edge of the culling domain (0.999
    cull_reach): for every record whose f64 quadratic reports t, both forms of the box test pass
    with the limit t_limit(t) and an entry t <= that limit, on the f32 box and on its binary16
    rounding; the compact entries give the code and a t no larger back.  OFFSETS has 4 of 7 aims
    within the radius, and origins inside the sphere always hit: at least a third report."""
    rng = np.random.default_rng(int(E) + 1)
    for bound in (10.0, 0.999 * lr.cull_reach(0.0)):
        o, d, c, r, ext = _aimed(rng, E, 60_000, bound)
        n = _check_must_hit(gpu_ctx, o, d, c, r, ext, lr.cull_reach(ext))
        print(f"E={E:g} origins within {bound:g} (1 + ext): {n} of {len(r)} records report a hit")
        assert len(r) > 54_000 and n > len(r) // 3


@pytest.mark.parametrize("E", [1.0, 1e3, 1e6])
def test_rays_that_miss_the_inflated_box_are_culled(gpu_ctx, E):
    """Tightness: origins within 10 (1 + ext), no limit.  Where the exact slab interval on the box
    inflated by 1e-3 (1 + ext) is empty or behind the origin, both forms of the device's test say
    miss (a kBoxTol of 1e-2 would widen a box 10 (1 + ext) away by a hundred times that inflation;
    parity cannot see over-conservative culling).  The aims
    of the other tests moved out by 0, 1, 2, 4 or 16 times the inflation, so that many rays pass
    just inside and just outside the inflated box: at least a quarter miss it."""
    rng = np.random.default_rng(int(E) + 11)
    o, d, c, r, ext = _aimed(rng, E, 120_000, 10.0, beyond=np.array([0.0, 1.0, 2.0, 4.0, 16.0]))
    pad = far_scenes.PAD * (1.0 + ext)
    rays = np.concatenate([o, d], axis=1)
    inf = np.full(len(r), np.inf)
    b32 = _boxes(c, r, pad)
    for name, box in [("f32", b32)] + ([("binary16", _half_boxes(b32))] if np.abs(b32).max() < 65504.0 else []):
        # (a binary16 box is compared with its own inflation: the rounding to a half is the host's)
        empty = _exact_slab_empty(o, d, box, 1e-3 * (1.0 + ext))
        out = gpu_ctx.cull_check(rays, box, inf, np.zeros(len(r), np.int32), lr.cull_reach(ext))
        print(f"E={E:g} {name}: {empty.sum()} of {len(r)} records miss the inflated box; the device accepts "
              f"{(empty & out['hit']).sum()} (box_hit), {(empty & out['hit_nf']).sum()} (near/far)")
        assert empty.sum() > len(r) // 4
        assert not (empty & out["hit"]).any() and not (empty & out["hit_nf"]).any()


def test_t_limit_bounds(gpu_ctx):
    """t_limit(rb, t) >= t 2^te as reals and <= t 2^te (1 + 3e-5), t 2^te across every f32 binade
    (2^-149 .. 2^127), for te = 0 (unit direction), 31 (|d| = 2^30) and -39 (|d| = 2^-40).  Below the
    normal range an f32 cannot follow an arbitrary t that closely, so there the upper bound is
    asserted for the f32 values themselves and only the lower one in between.  A value whose limit
    overflows f32 gives +inf."""
    rng = np.random.default_rng(5)
    e = np.repeat(np.arange(-149, 128), 24)
    m = np.where(np.arange(len(e)) % 24 == 0, 1.0, 1.0 + rng.random(len(e)))
    m[np.arange(len(e)) % 24 == 1] = 2.0 - 2.0 ** -30               # just below the next binade
    m[np.arange(len(e)) % 24 == 2] = 1.0 + 2.0 ** -23               # an f32 neighbour of the binade's start
    m[np.arange(len(e)) % 24 == 3] = 1.0 + 2.0 ** -24               # halfway to it
    s = np.ldexp(m, e)
    fmax = float(np.finfo(np.float32).max)
    s = np.concatenate([s, [fmax, fmax * (1 + 2.0 ** -25), 3.5e38, 1e39, 1e300]])
    with np.errstate(over="ignore"):
        f32_exact = s.astype(np.float32).astype(np.float64) == s
    denormal = s < 2.0 ** -126
    for scale, te in ((1.0, 0), (2.0 ** 30, 31), (2.0 ** -40, -39)):
        with np.errstate(over="ignore"):
            t = np.ldexp(s, -te)                # (1e300 2^39 is +inf: no limit)
        n = len(t)
        rays = np.zeros((n, 6))
        rays[:, 3] = scale
        out = gpu_ctx.cull_check(rays, np.zeros((n, 6), np.float32), t, np.zeros(n, np.int32))
        assert (out["te"] == te).all()
        lim = out["tlim"].astype(np.float64)
        assert (lim >= s).all(), (te, s[lim < s][:4], lim[lim < s][:4])
        overflow = s * (1.0 + 1.01e-5) > fmax
        assert np.isinf(lim[s > fmax]).all()
        tight = ~overflow & (~denormal | f32_exact)
        assert tight.sum() > 6000
        assert (lim[tight] <= s[tight] * (1.0 + 3e-5)).all(), (te, s[tight][lim[tight] > s[tight] * (1 + 3e-5)][:4])
    # no limit stays no limit
    out = gpu_ctx.cull_check(np.array([[0, 0, 0, 1.0, 0, 0]]), np.zeros((1, 6), np.float32), [np.inf], [0])
    assert np.isinf(out["tlim"][0]) and out["tlim"][0] > 0


def _far_records(rng, E, mul, n_spheres=300, per=40):
    """The far-camera family of test_lightgrid.py: spheres of radius 1e-5..1e-3 (1 + E) within
    [-E, E]^3, origins mul (1 + E) out along an axis (+-x, +-y, +-z in turn; the other two
    coordinates within the scene, or within 1e-4 of that distance), rays aimed within the radius at
    which a hit can still be reported: every ray is nearly axis-parallel."""
    c, r = far_scenes.cloud(E, n_spheres, int(np.log10(mul)) + int(E))
    ext = far_scenes.extent(c, r)
    k = np.repeat(np.arange(n_spheres), per)
    D = mul * (1.0 + E)
    axis = np.arange(len(k)) % 6
    # (lateral coordinates of at least 1e-4 D: from 1e9 away a ray closer to the axis has d . d = 1 and
    # d . oc = D exactly, its discriminant is exactly 0 and the reference reports nothing)
    o = rng.uniform(-1.0, 1.0, (len(k), 3)) * max(ext, 1e-4 * D)
    o[np.arange(len(k)), axis % 3] = np.where(axis < 3, D, -D)
    off = rng.random(len(k)) * far_scenes.phantom_radius(r[k], D)
    d = far_scenes.aim(rng, o, c, r, k, off)
    return o, d, c[k], r[k], ext


@pytest.mark.parametrize("E", [1.0, 1e3])
@pytest.mark.parametrize("mul", [1e4, 1e5, 1e6, 1e9])
def test_far_origins_are_not_culled(gpu_ctx, E, mul):
    """Origins mul (1 + E) away, far beyond cull_reach: every reported hit passes both forms of the
    box test (the null ray image: entry t 0), most of them hits that lie outside the padded box.
    Reported hits / of them outside the padded box, of 12000 records, when written (E = 1, E = 1e3):
    1e4: 4126 / 65, 3866 / 103; 1e5: 871 / 176, 904 / 174; 1e6: 976 / 245, 1032 / 266; 1e9: 994 / 290,
    927 / 275.  The same records with the rule switched off (reach +inf: the arithmetic before the
    rule) are printed, not asserted: how many reported hits the slab test alone would cull."""
    rng = np.random.default_rng(int(np.log10(mul)))
    o, d, c, r, ext = _far_records(rng, E, mul)
    t = _quadratic(o, d, c, r)
    pad = far_scenes.PAD * (1.0 + ext)
    outside = 0
    rep = np.nonzero(np.isfinite(t))[0]
    for i in rep:
        outside += bool(far_scenes.miss_distance(o[i], d[i], c[i:i + 1])[0] > np.sqrt(3.0) * (r[i] + pad))
    n = _check_must_hit(gpu_ctx, o, d, c, r, ext, lr.cull_reach(ext))
    out = gpu_ctx.cull_check(np.concatenate([o, d], axis=1), _boxes(c, r, pad), t, np.zeros(len(t), np.int32), lr.cull_reach(ext))
    assert (out["tnear"] == 0).all() and (out["te"] == 0).all()
    off = gpu_ctx.cull_check(np.concatenate([o, d], axis=1), _boxes(c, r, pad), t, np.zeros(len(t), np.int32))
    culled = np.isfinite(t) & ~(off["hit"] & (off["tnear"] <= off["tlim"]))
    print(f"FAR E={E:g} mul={mul:g}: {n} of {len(t)} report a hit, {outside} outside the padded box; without the rule "
          f"the slab test culls {culled.sum()} of them")
    assert n >= 400 and outside >= {1e4: 30, 1e5: 80, 1e6: 120, 1e9: 130}[mul]      # about half of the reference's


@pytest.mark.parametrize("E", [1.0, 1e3])
def test_edge_of_the_culling_domain(gpu_ctx, E):
    """An origin coordinate one part in 1e6 inside cull_reach(ext): the slab test is active (entry
    t > 0 for boxes ahead) and exact (reported hits pass); one part in 1e6 outside: the null image."""
    rng = np.random.default_rng(3)
    c, r = far_scenes.cloud(E, 300, 17)
    ext = far_scenes.extent(c, r)
    reach = lr.cull_reach(ext)
    k = np.repeat(np.arange(300), 40)
    for D, inside in ((reach * (1 - 1e-6), True), (reach * (1 + 1e-6), False)):
        axis = np.arange(len(k)) % 6
        o = rng.uniform(-ext, ext, (len(k), 3))
        o[np.arange(len(k)), axis % 3] = np.where(axis < 3, D, -D)
        d = far_scenes.aim(rng, o, c, r, k, rng.random(len(k)) * 0.9 * r[k])
        n = _check_must_hit(gpu_ctx, o, d, c[k], r[k], ext, reach)
        out = gpu_ctx.cull_check(np.concatenate([o, d], axis=1), _boxes(c[k], r[k], far_scenes.PAD * (1 + ext)),
                                 np.full(len(k), np.inf), np.zeros(len(k), np.int32), reach)
        assert n > 3000
        if inside:
            assert (out["tnear"] > 0.9 * (D - ext)).all() and out["hit"].all()
        else:
            assert (out["tnear"] == 0).all() and out["hit"].all() and out["hit_nf"].all()


def test_far_origin_near_the_end_of_the_f32_range(gpu_ctx):
    """Origins up to 1e38, still finite as f32: the null image, entry t = 0 (an origin beyond the f32
    range is outside what the slab tests support)."""
    rays = np.array([[0.0, 0.0, 1e38, 0.0, 0.0, -1.0], [-1e30, 2.0, 3.0, 1.0, 0.0, 0.0],
                     [5.0, -3e38, 0.0, 0.0, 1e-35, 0.0], [1.0, 1e12, 0.0, 0.0, -5e6, 0.0]])
    box = np.tile(np.array([[-1, -1, -1, 1, 1, 1]], np.float32), (4, 1))
    out = gpu_ctx.cull_check(rays, box, [np.inf, 5.0, np.inf, 1e30], [7, -7, 100, -100], lr.cull_reach(1.0))
    assert out["hit"].all() and out["hit_nf"].all()
    for k in ("tnear", "tnear_nf", "t16", "t18"):
        assert (out[k] == 0).all(), (k, out[k])
    assert out["node16"].tolist() == [7, -7, 100, -100] == out["node18"].tolist()
