"""The first-hit feature buffers (include/raytrace_amd.h, rt_render_aov) restated in Python, from the
oracle's exported building blocks only -- a helper of test_aov_model.py (which pins it against the
oracle's renders) and test_gpu_aov.py (which compares the device with it, bit for bit).

  camera       ref64.camera_build (camera.rs:51-73) gives position and matrix
  keys         kmix / key_child / key_pixel / key_f64 of trace_rng.hpp "keyed RNG", here in
               64-bit-masked Python ints and Python floats
  pixel -> ray main.rs:39-41, 50-53, then matrix * (px, py, 1) and v / sqrt(sqnorm) per component
               (camera.rs:78), in Python floats
  shapes       ref64.plane_intersect for every (ray, plane); for the spheres a numpy restatement
               of shapes.rs:50-89 over all rays at once (sphere_hits), which test_aov_model.py
               compares with ref64.sphere_intersect on every ray of a scene, bit for bit
  intersect    scene.rs:223-249: the objects in file order, the first strict minimum stays, the
               first NaN t beats everything
  average      main.rs:47-56: sum = 0.0; sum = sum + v_a in sample order; (float)(sum / spp)

numpy's float64 +, -, *, / and sqrt are the IEEE operations, one rounding each (no contraction: each
is a ufunc call of its own), so the vectorised parts compute what the scalar statements would.
"""
import copy
import functools
import math
import struct

import numpy as np

from libraytrace import scenes
from oracle import ref64

import adversarial_scenes
import far_scenes

M64 = 0xFFFFFFFFFFFFFFFF
CENTER, RANDOM = 0, 1
CASES = [(1, CENTER), (3, CENTER), (4, RANDOM)]        # (spp, jitter) every scene is checked with
SEEDS = (7, 0x5EED5EED5EED)


# ---- keyed RNG (trace_rng.hpp) ---------------------------------------------------------------
def kmix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key_child(k, i):
    return kmix((k + (i + 1) * 0x9E3779B97F4A7C15) & M64)


def key_pixel(seed, x, y):
    return kmix((kmix(seed & M64) + ((y << 32) | x)) & M64)


def key_f64(k, ident):
    bits = kmix(k ^ (((ident + 1) * 0xD1B54A32D192ED03) & M64))
    return struct.unpack("<d", struct.pack("<Q", 0x3FF0000000000000 | (bits & 0xFFFFFFFFFFFFF)))[0] - 1.0


# ---- pixel -> camera ray ---------------------------------------------------------------------
def camera_rays(spec, jitter, seed, sample):
    """(origin (3,), directions [height, width, 3]) of AA sample `sample` of every frame pixel."""
    pos, m = ref64.camera_build(spec.camera)
    hw, hh = float(spec.width) / 2.0, float(spec.height) / 2.0                    # main.rs:39-41
    scale = max(1.0 / hw, 1.0 / hh)
    d = np.empty((spec.height, spec.width, 3), np.float64)
    for y in range(spec.height):
        for x in range(spec.width):
            jx = jy = 0.5
            if jitter == RANDOM:
                ka = key_child(key_pixel(seed, x, y), sample)
                jx, jy = key_f64(ka, 0), key_f64(ka, 1)
            px = ((float(x) + jx) - hw) * scale                                   # main.rs:50-53
            py = ((float(y) + jy) - hh) * scale
            vx = m[0] * px + m[1] * py + m[2] * 1.0
            vy = m[3] * px + m[4] * py + m[5] * 1.0
            vz = m[6] * px + m[7] * py + m[8] * 1.0
            n = math.sqrt(vx * vx + vy * vy + vz * vz)
            d[y, x] = (vx / n, vy / n, vz / n)
    return np.array(pos, np.float64), d


# ---- shapes ----------------------------------------------------------------------------------
def sphere_hits(center, radius, o, d):
    """shapes.rs:50-89 for rays (o (3,), d [n, 3]) -> (hit [n] bool, t [n], normal [n, 3])."""
    c = [float(v) for v in center]
    radius = float(radius)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    ocx, ocy, ocz = o[0] - c[0], o[1] - c[1], o[2] - c[2]
    with np.errstate(all="ignore"):
        a = dx * dx + dy * dy + dz * dz
        b = 2.0 * (dx * ocx + dy * ocy + dz * ocz)
        cc = (ocx * ocx + ocy * ocy + ocz * ocz) - radius * radius
        disc = b * b - 4.0 * a * cc
        pos = disc > 0.0
        s = np.sqrt(np.where(pos, disc, 0.0))
        t1 = (-b - s) / (2.0 * a)
        t2 = (-b + s) / (2.0 * a)
        first = pos & (t1 > 0.0)
        hit = first | (pos & (t2 > 0.0))
        t = np.where(first, t1, t2)
        ux, uy, uz = (o[0] + dx * t) - c[0], (o[1] + dy * t) - c[1], (o[2] + dz * t) - c[2]    # ray.cast(t) - centre
        ln = np.sqrt(ux * ux + uy * uy + uz * uz)
        n = np.stack([ux / ln, uy / ln, uz / ln], axis=1)
    return hit, t, n


def plane_hits(point, normal, o, d):
    """ref64.plane_intersect (shapes.rs:100-112) ray by ray."""
    n = d.shape[0]
    hit, t = np.zeros(n, bool), np.zeros(n, np.float64)
    nrm = np.zeros((n, 3), np.float64)
    ot = tuple(o)
    for k in range(n):
        r = ref64.plane_intersect(point, normal, ot, tuple(d[k]))
        if r is not None:
            hit[k], t[k], nrm[k] = True, r[0], r[1]
    return hit, t, nrm


# ---- Scene::intersect and the per-sample values ----------------------------------------------
def first_hits(spec, o, dirs):
    """scene.rs:223-249 for rays (o, dirs [..., 3]) -> per ray: object id (-1: miss), t, the oriented
    normal, the hit object's diffuse (zeros for a miss)."""
    shape = dirs.shape[:-1]
    d = dirs.reshape(-1, 3)
    n = d.shape[0]
    obj = np.full(n, -1, np.int32)
    best_t = np.zeros(n, np.float64)
    best_n = np.zeros((n, 3), np.float64)
    best_nan = np.zeros(n, bool)
    for i, ob in enumerate(spec.objects):
        if ob["shape"] == "sphere":
            hit, t, nrm = sphere_hits(ob["center"], ob["radius"], o, d)
        else:
            hit, t, nrm = plane_hits(ob["point"], ob["normal"], o, d)
        cnan = np.isnan(t)
        with np.errstate(invalid="ignore"):
            better = hit & ((obj < 0) | (~best_nan & (cnan | (t < best_t))))
        obj[better] = i
        best_t[better] = t[better]
        best_n[better] = nrm[better]
        best_nan[better] = cnan[better]
    has = obj >= 0
    with np.errstate(invalid="ignore"):
        flip = has & ((best_n[:, 0] * d[:, 0] + best_n[:, 1] * d[:, 1]) + best_n[:, 2] * d[:, 2] > 0.0)    # raytrace.rs:38
    best_n[flip] = -best_n[flip]
    diffuse = np.array([[float(v) for v in ob["material"].get("diffuse", (0, 0, 0))] for ob in spec.objects] or
                       [[0.0, 0.0, 0.0]], np.float64)
    alb = np.where(has[:, None], diffuse[np.maximum(obj, 0)], 0.0)
    return {"object": obj.reshape(shape), "t": np.where(has, best_t, 0.0).reshape(shape),
            "normal": np.where(has[:, None], best_n, 0.0).reshape(shape + (3,)), "albedo": alb.reshape(shape + (3,)),
            "coverage": has.astype(np.float64).reshape(shape)}


def _spec_key(spec):
    return spec.to_text()


_CACHE = {}


def samples(spec, jitter, seed, n):
    """The per-sample values of samples 0 .. n-1 of every frame pixel (centre jitter: one evaluation)."""
    out = []
    for a in range(n):
        key = (_spec_key(spec), jitter, seed if jitter == RANDOM else 0, a if jitter == RANDOM else 0)
        if key not in _CACHE:
            o, d = camera_rays(spec, jitter, seed, a)
            _CACHE[key] = first_hits(spec, o, d)
        out.append(_CACHE[key])
    return out


def aov(spec, spp, jitter, seed):
    """The buffers of the whole frame as rt_render_aov defines them: depth, coverage float32 [h, w], normal,
    albedo float32 [h, w, 3], object int32 [h, w]."""
    per = samples(spec, jitter, seed, spp)
    out = {}
    for name, src in (("depth", "t"), ("normal", "normal"), ("albedo", "albedo"), ("coverage", "coverage")):
        acc = np.zeros_like(per[0][src])                        # main.rs:47
        with np.errstate(invalid="ignore"):
            for s in per:
                acc = acc + s[src]                                  # main.rs:48-55
            out[name] = (acc / float(spp)).astype(np.float32)       # main.rs:56, one rounding to f32
    out["object"] = per[0]["object"].copy()
    return out


# ---- the flat scenes that pin the model against the oracle's renders ---------------------------
def flat(spec, ambient_of, antialias):
    """Same geometry, camera and size; every object phong(0, 0, 1, ambient_of(i, object)), no lights, solid
    black background: by raytrace.rs:32-36 a pixel is sum(ambient of the sample's hit, or 0) / antialias."""
    f = copy.deepcopy(spec)
    f.lights, f.skybox, f.background, f.antialias = [], None, (0.0, 0.0, 0.0), antialias
    for i, ob in enumerate(f.objects):
        ob["material"] = scenes.phong((0, 0, 0), (0, 0, 0), 1.0, ambient_of(i, spec.objects[i]))
    return f


def flat_albedo(spec, antialias):
    return flat(spec, lambda i, ob: tuple(float(v) for v in ob["material"].get("diffuse", (0, 0, 0))), antialias)


def flat_coverage(spec, antialias):
    return flat(spec, lambda i, ob: (1.0, 1.0, 1.0), antialias)


def flat_object(spec):
    return flat(spec, lambda i, ob: (float(i + 1), 0.0, 0.0), 1)


# ---- the scenes -------------------------------------------------------------------------------
def inside_sphere_scene():
    """The camera inside a large sphere (every ray leaves through its far side: the t2 branch of
    shapes.rs:75-80, a normal that points along the ray and is flipped) with smaller ones inside and outside."""
    s = scenes.SceneSpec(width=40, height=28, max_depth=3, background=(0.1, 0.1, 0.1), name="inside",
                         camera={"ctor": "new", "position": (0.5, 0.25, 1.0), "look": (0.1, -0.05, -1.0),
                                 "up": (0.0, 1.0, 0.0), "im_dist": 1.2})
    s.sphere((0.0, 0.0, 0.0), 6.0, scenes.phong((0.7, 0.6, 0.5), (0.2, 0.2, 0.2), 16.0, (0.02, 0.02, 0.02)))
    s.sphere((0.8, 0.2, -3.0), 0.7, scenes.fresnel((0.2, 0.5, 0.8), (0.6, 0.6, 0.6), 32.0, (0.0, 0.0, 0.01), 1.5))
    s.sphere((-1.5, -0.5, -4.0), 1.0, scenes.phong((0.9, 0.2, 0.2), (0.3, 0.3, 0.3), 8.0, (0.01, 0.0, 0.0)))
    s.sphere((0.0, 0.0, -9.0), 2.0, scenes.phong((0.1, 0.9, 0.1), (0.3, 0.3, 0.3), 8.0, (0.0, 0.01, 0.0)))   # outside
    s.point_light((0.0, 2.0, 0.0), (1.0, 1.0, 1.0))
    return s


def scene_list(sky_paths):
    """{name: SceneSpec}; sky_paths: six texture files for the skybox scene (scenes.write_ppm)."""
    return {
        "tiny": adversarial_scenes.tiny(),
        "nan_plane": adversarial_scenes.nan_plane_scene(),
        "axis_tie": adversarial_scenes.axis_tie_scene(),
        "coincident": adversarial_scenes.coincident_scene(),
        "extreme": adversarial_scenes.extreme_magnitudes_scene(),
        "stochastic": scenes.stochastic(width=48, height=32, dof=False),
        "skybox_chain": scenes.skybox_chain_scene(sky_paths, 48, 32),
        "random": scenes.random_spheres(64, 64, 48, 4, seed=9, plane=True, name="aov_rand"),
        "inside": inside_sphere_scene(),
        "far": far_scenes.telephoto(1e5, size=32),
    }


SCENE_NAMES = ("tiny", "nan_plane", "axis_tie", "coincident", "extreme", "stochastic", "skybox_chain", "random",
               "inside", "far")


def bits(a):
    """A float32 array as its bit patterns (NaNs compare by payload too)."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
