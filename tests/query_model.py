"""The ray queries (include/raytrace_amd.h, rt_query_nearest / rt_query_occluded) restated in Python for rays
with origins of their own -- a helper of test_query_model.py (which pins it against the oracle) and
test_gpu_query.py (which compares the device with it, bit for bit).

  shapes       aov_model.sphere_hits (the numpy restatement of shapes.rs:50-89 that test_aov_model.py pins), here
               with one origin per ray: the same ufuncs on arrays where that file passes scalars; plane_hits below
               restates shapes.rs:100-112 the same way.  test_query_model.py compares both with
               ref64.sphere_intersect / ref64.plane_intersect on every (ray, object) pair of its ray sets
  intersect    scene.rs:223-249, the fold of aov_model.first_hits: the objects in file order, the first strict
               minimum stays, the first NaN t beats everything
  occlusion    raytrace.rs:43-50: intersect(ray) is Some(h) and (no range, or h.t * h.t < range)
  ray sets     the rays the renderer really issues from a first hit: the shadow ray of every light
               (raytrace.rs:34, 41-43; scene.rs:125, 131-139) and the mirror ray (raytrace.rs:60-62); the same with
               scaled directions, at the edge of the direction's domain (2^+-256), and from far origins
"""
import numpy as np

import aov_model as am

EPS = 0.00001                      # raytrace.rs:43, 62
SCALES = (-40, -21, -20, -1, 0, 1, 20, 21, 40)


def as_rays(rays):
    return np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)


def sphere_hits(center, radius, o, d):
    """shapes.rs:50-89 for rays (o [n, 3], d [n, 3]) -> (hit [n] bool, t [n], normal [n, 3])."""
    return am.sphere_hits(center, radius, (o[:, 0], o[:, 1], o[:, 2]), d)


def plane_hits(point, normal, o, d):
    """shapes.rs:100-112 for rays (o [n, 3], d [n, 3]): t = n.(p - o) / n.d, None iff t <= 0 (a NaN t is a hit);
    the normal as in the file."""
    p = [float(v) for v in point]
    nv = [float(v) for v in normal]
    with np.errstate(all="ignore"):
        ex, ey, ez = p[0] - o[:, 0], p[1] - o[:, 1], p[2] - o[:, 2]
        t = ((nv[0] * ex + nv[1] * ey) + nv[2] * ez) / ((nv[0] * d[:, 0] + nv[1] * d[:, 1]) + nv[2] * d[:, 2])
        hit = ~(t <= 0.0)
    nrm = np.broadcast_to(np.array(nv, np.float64), (o.shape[0], 3)).copy()
    return hit, t, nrm


def object_hits(ob, o, d):
    if ob["shape"] == "sphere":
        return sphere_hits(ob["center"], ob["radius"], o, d)
    return plane_hits(ob["point"], ob["normal"], o, d)


def intersect(spec, rays):
    """scene.rs:223-249 per ray -> (object id [n] int32, -1: miss; t [n], NaN kept; normal [n, 3], the shape's)."""
    r = as_rays(rays)
    o, d = r[:, :3], r[:, 3:]
    n = r.shape[0]
    obj = np.full(n, -1, np.int32)
    best_t = np.zeros(n, np.float64)
    best_n = np.zeros((n, 3), np.float64)
    best_nan = np.zeros(n, bool)
    for i, ob in enumerate(spec.objects):
        hit, t, nrm = object_hits(ob, o, d)
        cnan = np.isnan(t)
        with np.errstate(invalid="ignore"):
            better = hit & ((obj < 0) | (~best_nan & (cnan | (t < best_t))))
        obj[better] = i
        best_t[better] = t[better]
        best_n[better] = nrm[better]
        best_nan[better] = cnan[better]
    return obj, best_t, best_n


def nearest(spec, rays):
    """rt_query_nearest: {t float64 [n] (+inf: miss), object int32 [n] (-1), normal float64 [n, 3] (0: miss)}."""
    obj, t, nrm = intersect(spec, rays)
    has = obj >= 0
    return {"t": np.where(has, t, np.inf), "object": obj, "normal": np.where(has[:, None], nrm, 0.0)}


def occluded(spec, rays, r2=None):
    """rt_query_occluded: uint8 [n]; r2 None: any hit occludes, else h.t * h.t < r2 (false for a NaN t)."""
    obj, t, _ = intersect(spec, rays)
    has = obj >= 0
    if r2 is None:
        return has.astype(np.uint8)
    with np.errstate(all="ignore"):
        return (has & (t * t < np.asarray(r2, np.float64))).astype(np.uint8)


def flip(normal, rays):
    """raytrace.rs:38: the normal negated where dot(normal, direction) > 0 (rt_render_aov's orientation)."""
    d = as_rays(rays)[:, 3:]
    n = np.array(normal, np.float64)
    with np.errstate(invalid="ignore"):
        f = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] > 0.0
    n[f] = -n[f]
    return n


# ---- ray sets -----------------------------------------------------------------------------------
def camera_set(spec):
    """(i) the centre-jitter camera rays of every frame pixel, row-major."""
    o, d = am.camera_rays(spec, am.CENTER, 0, 0)
    d = d.reshape(-1, 3)
    return np.concatenate([np.broadcast_to(o, d.shape), d], axis=1)


def light_rays(light, pt):
    """The shadow rays of raytrace.rs:41-43 from the points pt [m, 3] to one light -> (rays [m, 6], r2 [m], ranged):
    a point light's direction normalize(location - pt) with range location.sqdist(pt) (scene.rs:125), a directional
    light's -direction as written, no range (scene.rs:131-139)."""
    m = pt.shape[0]
    with np.errstate(all="ignore"):
        if light["kind"] == "point":
            lv = np.array([float(v) for v in light["location"]], np.float64)
            vx, vy, vz = lv[0] - pt[:, 0], lv[1] - pt[:, 1], lv[2] - pt[:, 2]
            r2 = (vx * vx + vy * vy) + vz * vz
            ln = np.sqrt(r2)
            ldir = np.stack([vx / ln, vy / ln, vz / ln], axis=1)
            ranged = True
        else:
            lv = np.array([float(v) for v in light["direction"]], np.float64)
            ldir = np.broadcast_to(-lv, (m, 3)).copy()
            r2 = np.zeros(m, np.float64)
            ranged = False
        org = pt + ldir * EPS
    return np.concatenate([org, ldir], axis=1), r2, ranged


def surface_set(spec, cam=None):
    """(ii) from every first hit of the camera rays: the shadow ray to each point and directional light, with its
    range (+inf for a directional light: every hit is within it), and the mirror ray (raytrace.rs:60-62).
    -> (rays [m, 6], r2 [m]).  Hits with a NaN t have no finite point and are left out."""
    cam = camera_set(spec) if cam is None else cam
    obj, t, nrm = intersect(spec, cam)
    keep = (obj >= 0) & np.isfinite(t)
    o, d, t, nrm = cam[keep, :3], cam[keep, 3:], t[keep], nrm[keep]
    with np.errstate(all="ignore"):
        pt = o + d * t[:, None]                                       # ray.cast(t), raytrace.rs:34
        dn = (d[:, 0] * nrm[:, 0] + d[:, 1] * nrm[:, 1]) + d[:, 2] * nrm[:, 2]
        rd = d - nrm * (2.0 * dn)[:, None]                            # raytrace.rs:60-61
        mirror = np.concatenate([pt + rd * EPS, rd], axis=1)
    rays, r2 = [mirror], [np.full(pt.shape[0], np.inf)]
    for L in spec.lights:
        if L["kind"] not in ("point", "directional"):
            continue
        lr_, lr2, ranged = light_rays(L, pt)
        rays.append(lr_)
        r2.append(lr2 if ranged else np.full(pt.shape[0], np.inf))
    rays, r2 = np.concatenate(rays), np.concatenate(r2)
    ok = in_domain(rays, r2)
    return rays[ok], r2[ok]


DIR_EXP = 256                      # the direction's largest component magnitude lies in [2^-256, 2^256]


def in_domain(rays, r2=None):
    """The domain of a ray as the header states it: six finite components, |origin| <= 1e30 on every axis, the
    direction's largest component magnitude in [2^-256, 2^256], r2 not NaN and >= 0.  The direction's bound is the
    culling's, not the exact tests': a sphere's f32 box holds every hit the quadratic can report only while d.d,
    b*b, 4a*c and the discriminant neither overflow nor lose bits to underflow (at 2^500, b*b = +inf makes the
    reference report a hit at t = +inf on a sphere behind the origin, which the tree sources cull).  (A mirror ray
    off a plane whose normal has length 1e25 starts 1e45 away: the renderer issues it, the queries do not promise it.)"""
    r = as_rays(rays)
    with np.errstate(invalid="ignore"):
        m = np.abs(r[:, 3:]).max(axis=1)
        ok = (np.isfinite(r).all(axis=1) & (np.abs(r[:, :3]).max(axis=1) <= 1e30) & (m >= 2.0 ** -DIR_EXP) &
              (m <= 2.0 ** DIR_EXP))
        if r2 is not None:
            ok &= np.asarray(r2) >= 0.0
    return ok


def scene_in_domain(spec):
    """The scene's side of the domain: the spheres' extent <= 1e30, every radius >= 1e-60."""
    sph = [ob for ob in spec.objects if ob["shape"] == "sphere"]
    return all(abs(float(ob["radius"])) >= 1e-60 for ob in sph) and extent(spec) <= 1e30


def extent(spec):
    """The spheres' extent: the largest |centre +- radius| (rt_cull_reach's argument); 0 without spheres."""
    e = [abs(c) + abs(float(ob["radius"])) for ob in spec.objects if ob["shape"] == "sphere" for c in map(float, ob["center"])]
    return max(e) if e else 0.0


def far_set(spec, cam=None):
    """(iv) the camera rays started 2^21 (1 + extent) back along their own line: beyond the culling domain
    (cull_reach = 32 (1 + extent)), where the quadratic's cancellation is worst."""
    cam = camera_set(spec) if cam is None else cam
    far = cam.copy()
    far[:, :3] = cam[:, :3] - cam[:, 3:] * (2.0 ** 21 * (1.0 + extent(spec)))
    return far


def edge_set(rays, r2):
    """The domain's edge: every direction rescaled by the power of two that puts its largest component's exponent
    at +256 (even rays: m in [2^255, 2^256)) or -256 (odd rays: m in [2^-256, 2^-255)); the range scales by
    2^-2k with it.  -> (rays, r2, k)"""
    m = np.abs(rays[:, 3:]).max(axis=1)
    e = np.frexp(m)[1]                                                   # m = f 2^e, f in [0.5, 1)
    target = np.where(np.arange(rays.shape[0]) % 2 == 0, DIR_EXP, -DIR_EXP + 1)
    k = target - e
    out = rays.copy()
    out[:, 3:] = np.ldexp(rays[:, 3:], k[:, None])
    with np.errstate(all="ignore"):
        return out, np.ldexp(r2, -2 * k), k


def scaled_set(rays, r2, seed=5):
    """(iii) per-ray direction scales 2^k, k from SCALES (both sides of the slab tests' 2^+-20 switch); the range
    r2 counts in t*t, so it scales by 2^-2k with the ray.  -> (rays, r2, k)."""
    rng = np.random.default_rng(seed)
    k = rng.choice(np.array(SCALES), rays.shape[0])
    out = rays.copy()
    out[:, 3:] = np.ldexp(rays[:, 3:], k[:, None])
    return out, np.ldexp(r2, -2 * k), k


def permuted(n, seed=9):
    """(v) a fixed permutation of n rays."""
    return np.random.default_rng(seed).permutation(n)
