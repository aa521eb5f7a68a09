"""Light-view grids (host_lightgrid.cpp) on the CPU: for every
point light and many shade points, each sphere whose exact f64 test blocks
the shadow ray (raytrace.rs:39-49: ray from p + 1e-5*l toward the light,
Some(t) with t*t < |L - p|^2; shapes.rs:50-89 quadratic in the device's
operation order) must be on the candidate list the grid hands the device for
that point (rt_light_grid_candidates mirrors the device lookup, f32 face
coordinates and early stop included).  Checked against the linear scan of
every sphere, the reference's own shadow query (scene.rs:247-249)."""
import numpy as np
import pytest

import libraytrace as lr
from libraytrace import scenes
import far_scenes


def _spheres(spec):
    c, r, ids = [], [], []
    for i, o in enumerate(spec.objects):
        if o["shape"] == "sphere":
            c.append(o["center"]); r.append(o["radius"]); ids.append(i)
    return np.array(c, np.float64), np.array(r, np.float64), np.array(ids)


def _blockers(c, r, ids, L, p):
    """Object ids whose exact test shadows p from point light L (every sphere tested)."""
    v = L - p
    r2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]          # location.sqdist(pt)
    ln = np.sqrt(r2)
    d = v / ln                                           # normalize
    o = p + d * 1e-5
    oc = o - c
    a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    b = 2.0 * (d[0] * oc[:, 0] + d[1] * oc[:, 1] + d[2] * oc[:, 2])
    cc = (oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1] + oc[:, 2] * oc[:, 2]) - r * r
    disc = b * b - (4.0 * a) * cc
    with np.errstate(invalid="ignore"):
        s = np.sqrt(np.where(disc > 0.0, disc, 0.0))
        t1 = (-b - s) / (2.0 * a)
        t2 = (-b + s) / (2.0 * a)
    t = np.where(t1 > 0.0, t1, t2)
    hit = (disc > 0.0) & (t > 0.0) & (t * t < r2)
    return set(ids[hit].tolist())


def _shade_points(c, r, rng, n):
    """Points on sphere surfaces (where shadow queries start) and in the open."""
    k = rng.integers(0, len(c), n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    on = c[k] + u * r[k][:, None]
    lo, hi = c.min(0) - 1.0, c.max(0) + 1.0
    free = lo + (hi - lo) * rng.random((n // 4, 3))
    return np.vstack([on, free])


def _check(spec, n_points=1500, seed=0, resolution=0):
    sc = lr.Scene.deserialize(spec.to_text())
    c, r, ids = _spheres(spec)
    rng = np.random.default_rng(seed)
    pts = _shade_points(c, r, rng, n_points)
    checked = 0
    for li, L in enumerate(spec.lights):
        if L["kind"] != "point":
            continue
        Lp = np.array(L["location"], np.float64)
        # also points right next to the light
        near = Lp + rng.normal(size=(50, 3)) * 1e-3
        allp = np.vstack([pts, near])
        cands, info = sc.light_grid_candidates(li, allp, resolution=resolution)
        assert info[0] > 0
        for p, cand in zip(allp, cands):
            if cand is None:            # the device tests every sphere
                continue
            missing = _blockers(c, r, ids, Lp, p) - set(cand.tolist())
            assert not missing, f"light {li} point {p.tolist()}: blockers {sorted(missing)} not listed"
            checked += 1
    return checked


def test_grid_lists_every_blocker_config3():
    assert _check(scenes.config3(64, 64)) > 2000


def test_grid_lists_every_blocker_adversarial_lights():
    """Lights inside the cloud, at a sphere's centre, on its surface, on a plane;
    spheres from 1e-3 to 1e3 (the scene of test_gpu_parity's grid test)."""
    s = scenes.SceneSpec(width=8, height=8, max_depth=2,
                         camera={"ctor": "new", "position": (0, 2, 12), "look": (0, -0.1, -1), "up": (0, 1, 0),
                                 "im_dist": 1.2})
    rng = scenes.SplitMix64(4242)
    for k in range(400):
        cen = (rng.uniform(-6, 6), rng.uniform(-2, 6), rng.uniform(-10, 2))
        kd = (rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9))
        s.sphere(cen, 10 ** rng.uniform(-3, -0.2), scenes.phong(kd, (0.3, 0.3, 0.3), 20.0, (0.01, 0.01, 0.01)))
    s.sphere((3.0, 1.0, -4.0), 0.8, scenes.phong((0.8, 0.8, 0.2), (0.4, 0.4, 0.4), 10.0, (0, 0, 0)))
    s.sphere((0.0, -1e3 - 2.5, -4.0), 1e3, scenes.phong((0.5, 0.5, 0.5), (0.2, 0.2, 0.2), 5.0, (0, 0, 0)))
    s.point_light((0.0, 2.0, -4.0), (0.6, 0.6, 0.6))
    s.point_light((3.0, 1.0, -4.0), (0.5, 0.2, 0.2))
    s.point_light((3.0, 1.8, -4.0), (0.2, 0.5, 0.2))
    s.point_light((-5.0, 0.5, -30.0), (0.2, 0.2, 0.5))
    assert _check(s, n_points=1200, seed=1) > 4000


def test_grid_lists_every_blocker_ten_thousand_spheres():
    assert _check(scenes.config4(32, 32), n_points=800, seed=2) > 1000


@pytest.mark.parametrize("R", [16, 40, 512])
def test_grid_resolution_does_not_matter(R):
    """Any forced resolution (tuning "light_grid_res") keeps every blocker listed."""
    assert _check(scenes.config3(32, 32), n_points=600, seed=3, resolution=R) > 500


def test_grid_sizes_config3():
    sc = lr.Scene.deserialize(scenes.config3(32, 32).to_text())
    _, info0 = sc.light_grid_candidates(0, np.zeros((0, 3)))
    _, info1 = sc.light_grid_candidates(1, np.zeros((0, 3)))
    print(f"C3 grids: light 0 R={info0[0]} cells={info0[1]}; light 1 R={info1[0]} cells={info1[1]}; "
          f"entries (both) {info0[2]}")
    assert 16 <= info0[0] <= 512 and 16 <= info1[0] <= 512


# ---- the camera's view grid (host_lightgrid.cpp build_view_grid) ----

def _camera_dirs(sc, W, H, rng, n):
    """Camera-ray directions exactly as camera_ray builds them (main.rs:50-53,
    camera.rs:78): random pixels with centre jitter, plus the frame's corners."""
    d = sc.desc()
    M = np.array(d.camera.matrix[:], np.float64).reshape(3, 3)
    hw, hh = W / 2.0, H / 2.0
    scale = max(1.0 / hw, 1.0 / hh)
    xs = np.concatenate([rng.integers(0, W, n), [0, W - 1, 0, W - 1]])
    ys = np.concatenate([rng.integers(0, H, n), [0, 0, H - 1, H - 1]])
    px = ((xs + 0.5) - hw) * scale
    py = ((ys + 0.5) - hh) * scale
    dx = M[0, 0] * px + M[0, 1] * py + M[0, 2] * 1.0
    dy = M[1, 0] * px + M[1, 1] * py + M[1, 2] * 1.0
    dz = M[2, 0] * px + M[2, 1] * py + M[2, 2] * 1.0
    l = np.sqrt(dx * dx + dy * dy + dz * dz)
    return np.stack([dx / l, dy / l, dz / l], 1), np.array(d.camera.position[:], np.float64)


def _hits(c, r, o, d):
    """Exact t of every sphere for one ray (shapes.rs:60-89 in the device's order), inf = miss."""
    oc = o - c
    a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    b = 2.0 * (d[0] * oc[:, 0] + d[1] * oc[:, 1] + d[2] * oc[:, 2])
    cc = (oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1] + oc[:, 2] * oc[:, 2]) - r * r
    disc = b * b - (4.0 * a) * cc
    with np.errstate(invalid="ignore"):
        s = np.sqrt(np.where(disc > 0.0, disc, 0.0))
        t1 = (-b - s) / (2.0 * a)
        t2 = (-b + s) / (2.0 * a)
    t = np.where(t1 > 0.0, t1, t2)
    return np.where((disc > 0.0) & (t > 0.0), t, np.inf)


def _check_view(spec, n_rays=3000, seed=0, resolution=0):
    """Every sphere whose exact hit t is <= the ray's nearest t (the winner and any
    tie) is on the ray's list with a distance bound <= t, so the device's early
    stop (bound > t_limit(best t) >= best t) cannot skip it."""
    sc = lr.Scene.deserialize(spec.to_text())
    c, r, ids = _spheres(spec)
    rng = np.random.default_rng(seed)
    dirs, pos = _camera_dirs(sc, spec.width, spec.height, rng, n_rays)
    cands, info = sc.view_grid_candidates(dirs, resolution=resolution)
    assert info[0] > 0
    hits = 0
    for d, cand in zip(dirs, cands):
        if cand is None:                 # the device tests every sphere
            continue
        t = _hits(c, r, pos, d)
        best = t.min()
        if not np.isfinite(best):
            continue
        listed = dict(zip(cand[0].tolist(), cand[1].tolist()))
        for k in np.nonzero(t <= best)[0]:
            oid = int(ids[k])
            assert oid in listed, f"dir {d.tolist()}: sphere {oid} (t={t[k]}) not listed"
            assert listed[oid] <= t[k], (oid, listed[oid], t[k])
        hits += 1
    return hits, info


def test_view_grid_lists_every_winner_config3():
    n, info = _check_view(scenes.config3(4096, 4096))
    assert n > 500 and info[2] > 0
    print(f"C3 view grid: R={info[0]} cells={info[1]} entries={info[2]}")


def test_view_grid_dense_view_and_ten_thousand_spheres():
    assert _check_view(scenes.config3(512, 512, view="dense"), seed=1)[0] > 1000
    assert _check_view(scenes.config4(1024, 1024), n_rays=1500, seed=2)[0] > 300


@pytest.mark.parametrize("R", [1, 16, 333, 2048])
def test_view_grid_resolution_does_not_matter(R):
    assert _check_view(scenes.config3(256, 256), n_rays=1500, seed=3, resolution=R)[0] > 300


def test_view_grid_camera_inside_spheres():
    """The camera inside two nested spheres and on a third one's surface (always
    list), spheres from 1e-3 to 1e3, rays along the axes."""
    s = scenes.SceneSpec(width=33, height=33, max_depth=2,
                         camera={"ctor": "new", "position": (0.0, 0.0, 0.0), "look": (0.0, 0.0, -1.0),
                                 "up": (0.0, 1.0, 0.0), "im_dist": 1.0})
    m = scenes.phong((0.5, 0.5, 0.5), (0.2, 0.2, 0.2), 10.0, (0, 0, 0))
    s.sphere((0.0, 0.0, 0.0), 50.0, m)
    s.sphere((0.1, 0.0, 0.0), 2.0, m)
    s.sphere((0.0, 0.0, -3.0), 3.0, m)
    rng = scenes.SplitMix64(77)
    for k in range(300):
        s.sphere((rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(-40, 5)), 10 ** rng.uniform(-3, 0.5), m)
    s.sphere((0.0, -1e3 - 5.0, 0.0), 1e3, m)
    assert _check_view(s, n_rays=2000, seed=4)[0] > 1000


# ---- far origins ("the far-origin rule"; far_scenes.py) ----
#
# From |oc| away the f64 quadratic reports hits up to 4 sqrt(2^-53) |oc| outside a sphere, far
# outside its padded box once |oc| >> 32 (1 + E); the linear scan takes them, so the grids may
# not drop them.  The property is about what that arithmetic reports (_hits / _blockers), not
# about the true geometry.  Every case also counts the reported hits that lie geometrically
# outside the padded box (the line passes the centre at more than sqrt(3) (r + pad), f64), so
# that it cannot go empty; the minima are about half of what the reference arithmetic gave
# when the cases were written (the docstrings hold the figures).

def _view_far(spec, dirs):
    """_check_view's assertions for the given unit directions; a direction without a list (the
    device tests every sphere) passes.  Returns (rays with a reported hit, of those without a
    list, of those whose winner lies outside its padded box)."""
    sc = lr.Scene.deserialize(spec.to_text())
    c, r, ids = _spheres(spec)
    pos = np.array(sc.desc().camera.position[:], np.float64)
    pad = far_scenes.PAD * (1.0 + far_scenes.extent(c, r))
    cands, info = sc.view_grid_candidates(dirs)
    hits = none = outside = 0
    for d, cand in zip(dirs, cands):
        t = _hits(c, r, pos, d)
        best = t.min()
        if not np.isfinite(best):
            continue
        hits += 1
        w = int(np.argmin(t))
        outside += bool(far_scenes.miss_distance(pos, d, c[w:w + 1])[0] > np.sqrt(3.0) * (r[w] + pad))
        if cand is None:
            none += 1
            continue
        listed = dict(zip(cand[0].tolist(), cand[1].tolist()))
        for k in np.nonzero(t <= best)[0]:
            oid = int(ids[k])
            assert oid in listed, f"dir {d.tolist()}: sphere {oid} (t={t[k]}) not listed"
            assert listed[oid] <= t[k], (oid, listed[oid], t[k])
    return hits, none, outside


def _light_far(spec, li, pts):
    """_check's assertion for the given shade points and light li.  Returns (points with a
    reported blocker, of those without a list, of those with a blocker outside its padded box)."""
    sc = lr.Scene.deserialize(spec.to_text())
    c, r, ids = _spheres(spec)
    pad = far_scenes.PAD * (1.0 + far_scenes.extent(c, r))
    Lp = np.array(spec.lights[li]["location"], np.float64)
    cands, info = sc.light_grid_candidates(li, pts)
    assert info[0] > 0
    pos_of = {int(i): k for k, i in enumerate(ids)}
    shadowed = none = outside = 0
    for p, cand in zip(pts, cands):
        b = _blockers(c, r, ids, Lp, p)
        if not b:
            continue
        shadowed += 1
        d = (Lp - p) / np.linalg.norm(Lp - p)
        kk = np.array([pos_of[i] for i in b])
        outside += bool(np.any(far_scenes.miss_distance(p, d, c[kk]) > np.sqrt(3.0) * (r[kk] + pad)))
        if cand is None:
            none += 1
            continue
        missing = b - set(cand.tolist())
        assert not missing, f"light {li} point {p.tolist()}: blockers {sorted(missing)} not listed"
    return shadowed, none, outside


_AXIS, _OBLIQUE = (0.0, 0.0, 1.0), (0.36, 0.48, 0.8)


def _far_camera_case(E, D, seed, toward=_AXIS):
    """300 spheres within [-E, E]^3, radii 1e-5..1e-3 (1 + E); a camera at D * toward looking at the
    origin; 20 rays per sphere aimed within the radius at which a hit can still be reported."""
    c, r = far_scenes.cloud(E, 300, seed)
    pos = tuple(D * x for x in toward)
    spec = far_scenes.cloud_spec(c, r, {"ctor": "new", "position": pos, "look": tuple(-x for x in toward),
                                        "up": (0.0, 1.0, 0.0), "im_dist": 1.0})
    rng = np.random.default_rng(seed + 1)
    k = np.repeat(np.arange(len(c)), 20)
    o = np.broadcast_to(np.array(pos), (len(k), 3))
    off = rng.random(len(k)) * np.sqrt(r[k] ** 2 + 4 * 2.2e-16 * D * D)
    return spec, far_scenes.aim(rng, o, c, r, k, off)


# (rays with a reported hit, winners outside their padded box) at least, per camera and D / (1 + E).
# On the axis at 1e9 every ray has d . d = 1 and d . oc = D exactly, the discriminant is exactly 0
# and the reference reports nothing at all: that case only checks that nothing is listed wrongly.
_FAR_VIEW_MIN = {(_AXIS, 1e3): (2500, 0), (_AXIS, 1e4): (1100, 30), (_AXIS, 1e5): (250, 90), (_AXIS, 1e6): (250, 130),
                 (_AXIS, 1e9): (0, 0), (_OBLIQUE, 1e3): (2500, 0), (_OBLIQUE, 1e4): (1100, 45),
                 (_OBLIQUE, 1e5): (250, 80), (_OBLIQUE, 1e6): (250, 110), (_OBLIQUE, 1e9): (1500, 700)}


@pytest.mark.parametrize("toward", [_AXIS, _OBLIQUE], ids=["axis", "oblique"])
@pytest.mark.parametrize("E", [1.0, 1e3])
@pytest.mark.parametrize("mul", [1e3, 1e4, 1e5, 1e6, 1e9])
def test_view_grid_far_camera(E, mul, toward):
    """A camera mul (1 + E) away.  Rays with a reported hit / winners outside their padded box, of 6000
    rays, when written (E = 1, E = 1e3): on the axis 1e3: 5071 / 0, 4933 / 0; 1e4: 2300 / 81, 2284 / 69;
    1e5: 537 / 181, 594 / 220; 1e6: 646 / 336, 575 / 279; 1e9: none reported.  Oblique 1e3: 5061 / 0,
    4997 / 0; 1e4: 2414 / 118, 2441 / 93; 1e5: 612 / 161, 616 / 184; 1e6: 901 / 325, 670 / 239; 1e9:
    3370 / 1440, 3376 / 1673.  Before the far-origin rule the grid listed such winners with a bound
    above their t or not at all (the first experiment, on the axis: 37 of 2262 rays at 1e4, 88 of 606
    at 1e5, 93 of 588 at 1e6); now a camera out there has no grid."""
    spec, dirs = _far_camera_case(E, mul * (1.0 + E), int(np.log10(mul)) + (100 if E > 1 else 0), toward)
    hits, none, outside = _view_far(spec, dirs)
    print(f"VIEW {'axis' if toward == _AXIS else 'oblique'} E={E:g} mul={mul:g}: {hits} {none} {outside}")
    assert hits >= _FAR_VIEW_MIN[toward, mul][0] and outside >= _FAR_VIEW_MIN[toward, mul][1]


def _far_shade_case(E, D, seed):
    """The same spheres, a point light at (0.3, 3, 0.2) (1 + E) / 2, shade points D behind a sphere
    as seen from the light, their shadow rays aimed as in _far_camera_case."""
    c, r = far_scenes.cloud(E, 300, seed)
    L = np.array([0.3, 3.0, 0.2]) * (1.0 + E) / 2.0
    spec = far_scenes.cloud_spec(c, r, dict(scenes.DEFAULT_CAMERA), lights=[L])
    rng = np.random.default_rng(seed + 1)
    k = np.repeat(np.arange(len(c)), 4)
    to = c[k] - L
    ell = np.linalg.norm(to, axis=1)
    u = np.cross(to / ell[:, None], rng.normal(size=to.shape))
    u /= np.linalg.norm(u, axis=1)[:, None]
    off = rng.random(len(k)) * np.sqrt(r[k] ** 2 + 4 * 2.2e-16 * D * D)
    pts = L + (to + u * off[:, None]) * ((D + ell) / ell)[:, None]      # the line L -> p passes c + u off
    return spec, pts


# (points with a reported blocker, of those with a blocker outside its padded box) at least
_FAR_LIGHT_MIN = {1e3: (450, 0), 1e4: (230, 15), 1e5: (60, 25), 1e6: (70, 35), 1e9: (600, 500)}


@pytest.mark.parametrize("E", [1.0, 1e3])
@pytest.mark.parametrize("mul", [1e3, 1e4, 1e5, 1e6, 1e9])
def test_light_grid_far_shade_points(E, mul):
    """Shade points mul (1 + E) behind the spheres.  Points with a reported blocker / with one outside
    its padded box, of 1200 points, when written (E = 1, E = 1e3): 1e3: 976 / 0, 954 / 0; 1e4: 474 / 30,
    475 / 36; 1e5: 149 / 63, 127 / 53; 1e6: 162 / 76, 153 / 81; 1e9: 1200 / 1106, 1200 / 1100.  Before the
    far-origin rule the device lit points the reference shadows (the first experiment: 38 of 734 at
    1e5, 354 of 713 at 1e6); now such a point tests every sphere."""
    spec, pts = _far_shade_case(E, mul * (1.0 + E), seed=int(np.log10(mul)) + (200 if E > 1 else 50))
    shadowed, none, outside = _light_far(spec, 0, pts)
    print(f"LIGHT E={E:g} mul={mul:g}: {shadowed} {none} {outside}")
    assert shadowed >= _FAR_LIGHT_MIN[mul][0] and outside >= _FAR_LIGHT_MIN[mul][1]


@pytest.mark.parametrize("E", [1.0, 1e3])
def test_grids_at_the_edge_of_the_culling_domain(E):
    """Just inside lr.cull_reach(E) culling is active (every ray and point gets a real list, and the
    lists hold every reported hit); just outside there is no list."""
    c, r = far_scenes.cloud(E, 300, seed=7)
    reach = lr.cull_reach(far_scenes.extent(c, r))
    assert 31.9 * (1.0 + E) < reach <= 32.0 * (1.0 + far_scenes.extent(c, r))
    rng = np.random.default_rng(8)
    k = np.repeat(np.arange(len(c)), 10)
    for D, inside in ((reach * (1 - 1e-6), True), (reach * (1 + 1e-6), False)):
        spec = far_scenes.cloud_spec(c, r, {"ctor": "new", "position": (0.0, 0.0, D), "look": (0.0, 0.0, -1.0),
                                            "up": (0.0, 1.0, 0.0), "im_dist": 1.0}, lights=[(0.3 * E, 3.0 * E, 0.2 * E)])
        o = np.broadcast_to(np.array([0.0, 0.0, D]), (len(k), 3))
        dirs = far_scenes.aim(rng, o, c, r, k, rng.random(len(k)) * 1.2 * r[k])
        hits, none, _ = _view_far(spec, dirs)
        assert hits > 1500 and none == (0 if inside else hits), (D, hits, none)
        # shade points behind the spheres, as seen from the light, their largest |coordinate| D
        L = np.array(spec.lights[0]["location"])
        to = c[k] + rng.normal(size=(len(k), 3)) * 0.5 * r[k][:, None] - L
        with np.errstate(divide="ignore"):
            scale = np.min(np.where(to > 0, (D - L) / to, (-D - L) / to), axis=1)
        pts = L + to * scale[:, None]
        shadowed, none, _ = _light_far(spec, 0, pts)
        assert shadowed > 300 and none == (0 if inside else shadowed), (D, shadowed, none)


def test_view_grid_telephoto_frame():
    """far_scenes.telephoto: 4004 camera directions of the 64 x 64 frame.  Winners outside their padded
    box, of the rays with a reported hit, when written: D = 1e4: 45 of 148; D = 1e5: 164 of 1736 (the
    first experiment found the winner unlisted, or listed with a bound above its t, for 21 of 132
    and 409 of 1668)."""
    for D, least in ((1e4, 20), (1e5, 80)):
        spec = far_scenes.telephoto(D)
        sc = lr.Scene.deserialize(spec.to_text())
        dirs, pos = _camera_dirs(sc, spec.width, spec.height, np.random.default_rng(11), 4000)
        hits, none, outside = _view_far(spec, dirs)
        print(f"telephoto D={D}: {hits} rays hit, {none} without a list, {outside} winners outside their box")
        assert outside >= least


def test_light_grid_floor_frame():
    """far_scenes.floor(1e6): the shade points are where the frame's 64 x 64 camera rays (pixel centres)
    meet the floor.  When written the reference shadowed 1998 of the 4096 points, 1330 of them by a
    sphere outside whose padded box the shadow ray passes (the first experiment: no blocker listed
    for 1494)."""
    spec = far_scenes.floor(1e6)
    sc = lr.Scene.deserialize(spec.to_text())
    d = sc.desc()
    M = np.array(d.camera.matrix[:], np.float64).reshape(3, 3)
    pos = np.array(d.camera.position[:], np.float64)
    ys, xs = np.mgrid[0:spec.height, 0:spec.width]
    px = ((xs.ravel() + 0.5) - spec.width / 2.0) * (1.0 / (spec.width / 2.0))
    py = ((ys.ravel() + 0.5) - spec.height / 2.0) * (1.0 / (spec.height / 2.0))
    dirs = np.stack([px, py, np.ones_like(px)], 1) @ M.T
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    t = (0.0 - pos[1]) / dirs[:, 1]                     # the plane y = 0 (shapes.rs:100-112)
    pts = pos + dirs * t[:, None]
    shadowed, none, outside = _light_far(spec, 0, pts)
    print(f"floor 1e6: {shadowed} points shadowed, {none} without a list, {outside} with a blocker outside its box")
    assert shadowed == 1998 and outside >= 650


def test_config3_rays_and_points_keep_their_lists():
    """The far-origin rule leaves the C3 workload alone: every camera direction and every shade
    point of test_*_config3 above gets a list, none the "test every sphere" answer."""
    spec = scenes.config3(4096, 4096)
    sc = lr.Scene.deserialize(spec.to_text())
    dirs, pos = _camera_dirs(sc, spec.width, spec.height, np.random.default_rng(0), 3000)
    cands, info = sc.view_grid_candidates(dirs)
    assert info[0] > 0 and all(cand is not None for cand in cands)
    c, r, ids = _spheres(spec)
    pts = _shade_points(c, r, np.random.default_rng(0), 1500)
    for li in range(len(spec.lights)):
        cands, info = sc.light_grid_candidates(li, pts)
        assert info[0] > 0 and all(cand is not None for cand in cands)
