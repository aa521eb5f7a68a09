"""The Python model of the ray queries (tests/query_model.py) pinned against the oracle, before any device is
compared with it (test_gpu_query.py); no GPU.

  building blocks   the numpy restatements of the sphere and the plane test equal ref64.sphere_intersect /
                    ref64.plane_intersect bit for bit (a NaN by its position) on every (ray, object) pair of the
                    camera, surface, scaled, domain-edge and far-origin ray sets of seven scenes
  nearest           on camera rays it is aov_model.first_hits (which test_aov_model.py pins to the oracle's renders)
  occlusion         a scene with ambient 0, white diffuse, no specular, depth 0 and one light: by raytrace.rs:32-56
                    the oracle's pixel is exactly 0 iff its shadow ray is occluded or the clamped cosine is 0
  scaling           a direction times 2^k gives the same object and t 2^-k, bit for bit

Also here: the planner's cases (tests/native/query_plan_check.cpp, built with sanitizers as a stand-alone program,
as test_aov_model.py builds its own), and what the binding declares.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import libraytrace as lr
from libraytrace import scenes
from oracle import ref64

import aov_model as am
import query_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-raytrace_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
CXXFLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-O1", "-g", "-I" + CSRC,
            "-I" + os.path.join(ROOT, "include")]
SAN = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
BLOCK_SCENES = ("tiny", "nan_plane", "axis_tie", "coincident", "extreme", "inside", "far")


@pytest.fixture(scope="module")
def specs(tmp_path_factory):
    d = tmp_path_factory.mktemp("query_sky")
    paths = [str(d / f"f{k}.ppm") for k in range(6)]
    for p, f in zip(paths, scenes.skybox_faces(size=8, seed=2)):
        scenes.write_ppm(p, f)
    return am.scene_list(paths)


def ray_sets(spec):
    """(rays, r2): the camera rays (i), the surface rays (ii), both with scaled directions (iii) and with directions
    at the edge of the domain, and the camera rays from far origins (iv)."""
    cam = qm.camera_set(spec)
    sur, r2 = qm.surface_set(spec, cam)
    base = np.concatenate([cam, sur])
    base_r2 = np.concatenate([np.full(cam.shape[0], np.inf), r2])
    scaled, scaled_r2, _ = qm.scaled_set(base, base_r2)
    edge, edge_r2, _ = qm.edge_set(base, base_r2)
    far = qm.far_set(spec, cam)
    assert qm.scene_in_domain(spec)
    return (np.concatenate([base, scaled, edge, far]),
            np.concatenate([base_r2, scaled_r2, edge_r2, np.full(far.shape[0], np.inf)]))


def same64(a, b):
    """float64 arrays equal in every bit, NaNs by position (IEEE leaves a NaN's sign and payload open)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


# ---- building blocks ---------------------------------------------------------------------------

# the oracle's exported shape tests through a second handle of the same library, so that a call takes raw addresses
# into the numpy arrays (ref64.sphere_intersect builds three ctypes arrays per call: millions of pairs here)
_ORACLE = C.CDLL(ref64.LIB_PATH)
_ORACLE.ref_sphere_intersect.restype = C.c_int
_ORACLE.ref_sphere_intersect.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_ORACLE.ref_plane_intersect.restype = C.c_int
_ORACLE.ref_plane_intersect.argtypes = [C.c_void_p] * 6


def oracle_object(ob, rays):
    """ref_sphere_intersect / ref_plane_intersect of one object on every ray -> (hit, t, normal)."""
    n = rays.shape[0]
    hit, t, nrm = np.zeros(n, bool), np.zeros(n, np.float64), np.zeros((n, 3), np.float64)
    base, tb, nb = rays.ctypes.data, t.ctypes.data, nrm.ctypes.data
    if ob["shape"] == "sphere":
        c = np.array([float(v) for v in ob["center"]], np.float64)
        r, ca, fn = float(ob["radius"]), c.ctypes.data, _ORACLE.ref_sphere_intersect
        for k in range(n):
            hit[k] = fn(ca, r, base + 48 * k, base + 48 * k + 24, tb + 8 * k, nb + 24 * k)
    else:
        p = np.array([float(v) for v in ob["point"]], np.float64)
        nv = np.array([float(v) for v in ob["normal"]], np.float64)
        pa, na, fn = p.ctypes.data, nv.ctypes.data, _ORACLE.ref_plane_intersect
        for k in range(n):
            hit[k] = fn(pa, na, base + 48 * k, base + 48 * k + 24, tb + 8 * k, nb + 24 * k)
    return hit, t, nrm


def test_fast_oracle_calls_are_the_oracles():
    """The raw-address calls above against ref64.sphere_intersect / plane_intersect themselves."""
    spec = am.inside_sphere_scene()
    spec.plane((0.0, -1.0, 0.0), (0.0, 2.0, 0.1), spec.objects[0]["material"])
    rays = np.ascontiguousarray(qm.camera_set(spec)[::7])
    for ob in spec.objects:
        hit, t, nrm = oracle_object(ob, rays)
        for k in range(rays.shape[0]):
            o, d = tuple(rays[k, :3]), tuple(rays[k, 3:])
            r = (ref64.sphere_intersect(ob["center"], ob["radius"], o, d) if ob["shape"] == "sphere"
                 else ref64.plane_intersect(ob["point"], ob["normal"], o, d))
            assert (r is not None) == bool(hit[k])
            if r is not None:
                assert same64([r[0]], [t[k]]) and same64(r[1], nrm[k])


@pytest.mark.parametrize("name", BLOCK_SCENES)
def test_numpy_shape_tests_are_the_oracles(specs, name):
    spec = specs[name]
    rays, _ = ray_sets(spec)
    rays = np.ascontiguousarray(rays)
    hits = nans = 0
    for i, ob in enumerate(spec.objects):
        hit, t, nrm = qm.object_hits(ob, rays[:, :3], rays[:, 3:])
        ohit, ot, onrm = oracle_object(ob, rays)
        assert np.array_equal(hit, ohit), (name, i, int((hit != ohit).sum()))
        assert same64(t[hit], ot[hit]), (name, i, "t")
        assert same64(nrm[hit], onrm[hit]), (name, i, "normal")
        hits += int(hit.sum())
        nans += int(np.isnan(t[hit]).sum())
    if name == "tiny":
        assert not spec.objects and rays.shape[0] == 4 * spec.width * spec.height
    else:
        assert hits > 100, (name, hits)
    if name == "nan_plane":
        assert nans > 0


def test_ray_sets_cover_what_they_are_for(specs):
    """Origins on surfaces, unnormalised directions on both sides of 2^+-20, origins beyond the culling domain."""
    rays, r2 = ray_sets(specs["extreme"])
    m = np.abs(rays[:, 3:]).max(axis=1)
    assert (m > 2.0 ** 20).any() and (m < 2.0 ** -20).any() and ((m > 0.5) & (m <= 1.0)).any()
    assert m.max() <= 2.0 ** 256 and m.min() >= 2.0 ** -256 and np.abs(rays[:, :3]).max() <= 1e30
    assert (m >= 2.0 ** 255).sum() > 1000 and (m < 2.0 ** -255).sum() > 1000       # the edge of the domain, both sides
    assert qm.in_domain(rays, r2).all()
    assert np.isfinite(rays).all() and not np.isnan(r2).any() and (r2 >= 0).all()
    assert np.isinf(r2).any() and np.isfinite(r2).any()
    far = qm.camera_set(specs["far"])
    c = np.array([ob["center"] for ob in specs["far"].objects], np.float64)
    rad = np.array([ob["radius"] for ob in specs["far"].objects], np.float64)
    ext = float(np.max(np.abs(np.concatenate([c - rad[:, None], c + rad[:, None]]))))
    assert np.abs(far[:, :3]).max() > lr.cull_reach(ext)                 # (iv): beyond the far-origin rule's reach
    # the extreme scene's directional light of magnitude 1e34 starts its shadow rays far outside too
    assert (np.abs(rays[:, :3]).max(axis=1) > 1e20).any()


# ---- nearest: camera rays against the AOV model -------------------------------------------------

@pytest.mark.parametrize("name", am.SCENE_NAMES)
def test_nearest_on_camera_rays_is_the_aov_model(specs, name):
    spec = specs[name]
    o, d = am.camera_rays(spec, am.CENTER, 0, 0)
    want = am.first_hits(spec, o, d)
    rays = qm.camera_set(spec)
    got = qm.nearest(spec, rays)
    obj = want["object"].reshape(-1)
    hit = obj >= 0
    assert np.array_equal(got["object"], obj)
    assert same64(got["t"][hit], want["t"].reshape(-1)[hit]) and np.isposinf(got["t"][~hit]).all()
    assert same64(qm.flip(got["normal"], rays), want["normal"].reshape(-1, 3))
    assert not got["normal"][~hit].any()
    # the shape's own normal is not oriented: inside the enclosing sphere it points along the ray
    if name == "inside":
        dots = (got["normal"] * rays[:, 3:]).sum(axis=1)
        assert (dots[obj == 0] > 0).all() and (obj == 0).sum() > 100


# ---- occlusion against the oracle's renders -------------------------------------------------------

WHITE = scenes.phong((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 1.0, (0.0, 0.0, 0.0))


def shadow_scene(light):
    """A floor, spheres between it and the light, and one sphere beyond the light as seen from the floor (its hit is
    farther than the point light: t * t < r2 is false, raytrace.rs:47); ambient 0, white diffuse, no specular."""
    s = scenes.SceneSpec(width=56, height=40, max_depth=0, background=(0.0, 0.0, 0.0), name="shadow_" + light,
                         camera={"ctor": "new", "position": (0.0, 2.5, 4.0), "look": (0.0, -0.35, -1.0),
                                 "up": (0.0, 1.0, 0.0), "im_dist": 1.1})
    s.plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), WHITE)
    s.sphere((0.0, 1.2, -3.0), 0.9, WHITE)
    s.sphere((-1.2, 1.0, -2.4), 0.6, WHITE)
    s.sphere((1.3, 1.1, -3.6), 0.5, WHITE)
    s.sphere((0.3, 0.3, -1.0), 0.3, WHITE)
    s.sphere((0.0, 7.0, -3.0), 2.5, WHITE)              # above the light: beyond it for every floor point below
    if light == "point":
        s.point_light((0.0, 3.2, -3.0), (1.0, 1.0, 1.0))
    else:
        s.directional_light((0.25, -1.0, 0.15), (1.0, 1.0, 1.0))
    return s


@pytest.mark.parametrize("light", ["point", "directional"])
def test_occlusion_is_the_oracles_shadow_test(light):
    spec = shadow_scene(light)
    assert len(spec.lights) == 1
    ref = ref64.render(spec, max_depth=0, jitter=0)["rgb64"].reshape(-1, 3)
    cam = qm.camera_set(spec)
    obj, t, nrm = qm.intersect(spec, cam)
    has = obj >= 0
    assert not ref[~has].any()                                           # the black background
    o, d = cam[has, :3], cam[has, 3:]
    pt = o + d * t[has][:, None]                                         # raytrace.rs:34
    normal = qm.flip(nrm[has], cam[has])                                 # raytrace.rs:38
    rays, r2, ranged = qm.light_rays(spec.lights[0], pt)                 # raytrace.rs:41-43, scene.rs:125
    occ = qm.occluded(spec, rays, r2 if ranged else None).astype(bool)
    ld = rays[:, 3:]
    cos = (ld[:, 0] * normal[:, 0] + ld[:, 1] * normal[:, 1]) + ld[:, 2] * normal[:, 2]
    dark = occ | ~(cos > 0.0)                                            # the clamped cosine is 0
    black = ~ref[has].any(axis=1)
    assert np.array_equal(black, dark), (light, int((black != dark).sum()))
    assert (ref[has][~black] > 0).all()
    assert occ.sum() > 50 and (~dark).sum() > 50                         # both outcomes occur
    if ranged:
        # the range decides: something is hit, but beyond the light
        anyhit = qm.occluded(spec, rays, None).astype(bool)
        decided = anyhit & ~occ
        assert decided.sum() > 20 and (~black[decided & (cos > 0.0)]).all() and (decided & (cos > 0.0)).sum() > 20
    else:
        assert np.array_equal(occ, qm.occluded(spec, rays, np.full(rays.shape[0], np.inf)).astype(bool))


def test_occlusion_edges_in_the_model(specs):
    """r2 = t*t is not occluded, the next double up is; 0 never, +inf whenever hit; a NaN t only without a range."""
    spec = specs["random"]
    rays = qm.camera_set(spec)
    got = qm.nearest(spec, rays)
    hit = got["object"] >= 0
    t = got["t"][hit]
    tt = t * t
    assert not qm.occluded(spec, rays[hit], tt).any()
    assert qm.occluded(spec, rays[hit], np.nextafter(tt, np.inf)).all()
    assert not qm.occluded(spec, rays, np.zeros(rays.shape[0])).any()
    assert np.array_equal(qm.occluded(spec, rays, np.full(rays.shape[0], np.inf)), hit.astype(np.uint8))
    spec = specs["nan_plane"]
    rays = qm.camera_set(spec)
    nan = np.isnan(qm.nearest(spec, rays)["t"])
    assert nan.any()
    assert qm.occluded(spec, rays)[nan].all()
    assert not qm.occluded(spec, rays, np.full(rays.shape[0], np.inf))[nan].any()


# ---- scaling identity ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["random", "extreme", "inside", "nan_plane"])
def test_scaling_a_direction_scales_t_exactly(specs, name):
    spec = specs[name]
    cam = qm.camera_set(spec)
    sur, _ = qm.surface_set(spec, cam)
    rays = np.concatenate([cam, sur])
    base = qm.nearest(spec, rays)
    rng = np.random.default_rng(3)
    for ks in (np.full(rays.shape[0], 40), np.full(rays.shape[0], -40), rng.integers(-40, 41, rays.shape[0])):
        sc = rays.copy()
        sc[:, 3:] = np.ldexp(rays[:, 3:], ks[:, None])
        got = qm.nearest(spec, sc)
        assert np.array_equal(got["object"], base["object"]), name
        assert same64(got["t"], np.ldexp(base["t"], -ks)), name
        assert same64(got["normal"], base["normal"]), name
    # ... and at the edge of the direction's domain, 2^+-256 (query_model.edge_set): still no over- or underflow
    sc, _, ks = qm.edge_set(rays, np.full(rays.shape[0], np.inf))
    got = qm.nearest(spec, sc)
    assert np.array_equal(got["object"], base["object"]) and same64(got["t"], np.ldexp(base["t"], -ks)), name
    assert same64(got["normal"], base["normal"]), name
    assert (base["object"] >= 0).sum() > 50


def test_beyond_the_direction_bound_the_reference_reports_hits_no_box_holds():
    """Why the domain stops at 2^+-256 and not at 2^+-500: at 2^500 b*b overflows, and the reference
    itself reports a hit at t = +inf on a sphere BEHIND the ray's origin, which no bounding box can hold.  At 2^256
    the same ray misses, as geometry says."""
    c, r, o = (-3000.0, 0.0, 0.0), 2500.0, (0.0, 0.0, 0.0)
    far = ref64.sphere_intersect(c, r, o, (2.0 ** 500, 0.0, 0.0))
    assert far is not None and far[0] == np.inf
    assert ref64.sphere_intersect(c, r, o, (2.0 ** 256, 0.0, 0.0)) is None
    assert ref64.sphere_intersect(c, r, o, (1.0, 0.0, 0.0)) is None
    rays = np.array([[0, 0, 0, 2.0 ** 500, 0, 0], [0, 0, 0, 2.0 ** 256, 0, 0]], np.float64)
    assert list(qm.in_domain(rays)) == [False, True]


# ---- the planner and the binding -------------------------------------------------------------------

def test_query_planner(tmp_path):
    exe = str(tmp_path / "query_plan_check")
    cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + SAN + ["-o", exe, os.path.join(NATIVE, "query_plan_check.cpp"),
                                                            os.path.join(CSRC, "render_plan.cpp")]
    cc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout
    assert "query_plan_check ok" in run.stdout


def test_entry_points_are_declared_and_exported():
    names = lr.header_functions()
    for fn in ("rt_query_nearest", "rt_query_occluded", "rt_query_nearest_device", "rt_query_occluded_device"):
        assert fn in names and hasattr(lr.lib, fn), fn
    assert lr.RT_ABI_VERSION == 10 == lr.lib.rt_abi_version()
    assert C.sizeof(lr.rt_hit_buffers) == 3 * C.sizeof(C.c_void_p)
    assert [f[0] for f in lr.rt_hit_buffers._fields_] == ["t", "object", "normal"]
    header = open(lr.HEADER_PATH).read()
    enum = re.search(r"enum rt_hit_channel \{([^}]*)\}", header).group(1)
    vals = {k: int(v) for k, v in re.findall(r"(RT_HIT_[A-Z]+)\s*=\s*(\d+)", enum)}
    assert vals == {"RT_HIT_T": lr.RT_HIT_T, "RT_HIT_OBJECT": lr.RT_HIT_OBJECT, "RT_HIT_NORMAL": lr.RT_HIT_NORMAL}
    assert lr.RT_HIT_ALL == lr.RT_HIT_T | lr.RT_HIT_OBJECT | lr.RT_HIT_NORMAL == 7
    assert re.search(r"typedef struct \{ double\* t; int32_t\* object; double\* normal; \} rt_hit_buffers;", header)
    assert re.search(r"#define RT_ABI_VERSION 10\b", header) and re.search(r"RT_KF_COUNT = 8\b", header)
    # a null context is refused before anything is touched
    b = lr.rt_hit_buffers()
    assert lr.lib.rt_query_nearest(None, None, 0, lr.RT_HIT_T, C.byref(b), 0, None) == lr.RT_E_INVALID
    assert lr.lib.rt_query_occluded(None, None, None, 0, None, 0, None) == lr.RT_E_INVALID
    assert lr.lib.rt_query_nearest_device(None, None, 0, lr.RT_HIT_T, C.byref(b), 0, None) == lr.RT_E_INVALID
    assert lr.lib.rt_query_occluded_device(None, None, None, 0, None, 0, None) == lr.RT_E_INVALID
