"""prim_model.py, the numpy restatement that test_gpu_prims.py holds the device to, pinned on the CPU to
the oracle's own building blocks: the intersections to ref_sphere_intersect / ref_plane_intersect on a
sample of every record class, the shading terms to ref_render's f64 colour of one-object, one-light,
one-pixel scenes; and the correctly rounded libm fixture (tests/golden/libm_cr.npz) to a recomputation."""
import math
import os
import sys

import numpy as np
import pytest

from libraytrace import scenes
from oracle import ref64

import aov_model
import prim_model as pm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def records():
    return pm.isect_records()


def _sample(labels, per_class, seed):
    rng = np.random.default_rng(seed)
    idx = []
    for name in np.unique(labels):
        k = np.flatnonzero(labels == name)
        idx.append(rng.choice(k, min(per_class, len(k)), replace=False))
    return np.sort(np.concatenate(idx))


def test_sphere_model_is_the_oracles_intersection_bit_for_bit(records):
    rays, sph, _, lab = records
    idx = _sample(lab, 500, 1)
    assert len(idx) >= 20000 and len(np.unique(lab)) >= 40
    m = pm.sphere(rays[idx, :3], rays[idx, 3:], sph[idx, :3], sph[idx, 3])
    assert m["hit"].sum() > 5000 and (~m["hit"]).sum() > 5000 and m["second"].sum() > 1000
    for j, i in enumerate(idx):
        r = ref64.sphere_intersect(sph[i, :3], sph[i, 3], rays[i, :3], rays[i, 3:])
        assert (r is not None) == m["hit"][j], (lab[i], rays[i], sph[i])
        if r is not None:
            got = np.concatenate([[m["t"][j]], m["n"][j]])
            assert pm.bits_equal(got, np.array([r[0], *r[1]])).all(), (lab[i], rays[i], sph[i], got, r)


def test_plane_model_is_the_oracles_intersection_bit_for_bit(records):
    rays, _, pl, lab = records
    idx = _sample(lab, 500, 2)
    assert len(idx) >= 20000
    m = pm.plane(rays[idx, :3], rays[idx, 3:], pl[idx, :3], pl[idx, 3:])
    for j, i in enumerate(idx):
        r = ref64.plane_intersect(pl[i, :3], pl[i, 3:], rays[i, :3], rays[i, 3:])
        assert (r is not None) == m["hit"][j], (lab[i], rays[i], pl[i])
        if r is not None:
            assert pm.bits_equal(np.array([m["t"][j]]), np.array([r[0]])).all(), (lab[i], rays[i], pl[i])
            assert pm.bits_equal(np.array(r[1]), pl[i, 3:]).all()


def test_records_meet_the_coverage_conditions(records):
    cov, _, _ = pm.coverage(*records)
    print(cov)
    for k, floor in pm.COVERAGE_FLOOR.items():
        assert cov[k] >= floor, (k, cov[k], floor)


# ---- shading: one sphere, one light, one pixel, depth 0 -------------------------------------------------
def _shading_scenes():
    rng = np.random.default_rng(20261022)
    out = []
    exps = [0.0, 1.0, 32.0, 2.5]
    for i in range(320):
        look = pm._unit(rng, 1)[0]
        pos = rng.uniform(-20.0, 20.0, 3)
        radius = 10.0 ** rng.uniform(-1.0, 1.0)
        centre = pos + look * (radius * rng.uniform(1.5, 6.0)) + pm._perp(rng, look[None])[0] * (radius * rng.uniform(0.0, 0.95))
        kd, ks, amb = rng.uniform(0.0, 1.0, 3), rng.uniform(0.0, 1.0, 3), rng.uniform(0.0, 0.3, 3)
        if i % 5 == 4:
            ks = ks * 1e-3                                   # the specular flag off, the diffuse one on
        mat = (scenes.fresnel(kd, ks, exps[i % 4], amb, [1.5, 1.0, 2.4, 1e3][(i // 16) % 4]) if (i // 4) % 2
               else scenes.phong(kd, ks, exps[i % 4], amb))
        spec = scenes.SceneSpec(width=1, height=1, antialias=1, max_depth=0, background=(0.1, 0.2, 0.3), name=f"prim{i}")
        spec.camera = {"ctor": "new", "position": tuple(pos), "look": tuple(look), "up": tuple(pm._perp(rng, look[None])[0]),
                       "im_dist": 1.0}
        spec.sphere(centre, radius, mat)
        # lights on the camera's side (lit), anywhere (about half of them behind the surface), far and near
        toward = pos if i % 3 else centre + pm._unit(rng, 1)[0] * radius * 10.0 ** rng.uniform(0.1, 3.0)
        lc = rng.uniform(0.2, 2.0, 3)
        if (i // 8) % 2:
            spec.directional_light((centre - toward) * 10.0 ** rng.uniform(-3.0, 3.0), lc)
        else:
            spec.point_light(toward + pm._unit(rng, 1)[0] * radius * 0.3, lc)
        out.append(spec)
    return out


def test_shading_model_is_the_oracles_colour_bit_for_bit():
    """The model's ambient + light (+ mirrored background) colour against ref_render's out_rgb64 of 320 scenes:
    Phong and Fresnel, point and directional lights, lit and back-facing (own-shadowed) hits, exponents 0, 1, 32
    and 2.5.  The power of the model's own cosine is the C library's pow, the oracle's, reached through math.pow:
    numpy's pow is not that function (its vector loops differ from it by one representable value on about
    4% of the fixture's operands, exponents 2 and 0.5 among them; its scalar path too), and scene 211 (exponent
    2.5) showed it.  So numpy's pow stays pinned on the exponents 0 and 1 only, where it must equal the C library's."""
    specs = _shading_scenes()
    n = len(specs)
    col = lambda f: np.array([f(s) for s in specs], np.float64)         # noqa: E731
    o = col(lambda s: s.camera["position"])
    d = np.array([aov_model.camera_rays(s, aov_model.CENTER, 0, 0)[1][0, 0] for s in specs])
    c, r = col(lambda s: s.objects[0]["center"]), col(lambda s: s.objects[0]["radius"])
    mt = [s.objects[0]["material"] for s in specs]
    kd, ks, amb = (np.array([m[k] for m in mt], np.float64) for k in ("diffuse", "specular", "ambient"))
    exponent = np.array([m["exponent"] for m in mt])
    ior = np.array([m.get("ior", 1.0) for m in mt])
    mat = np.array([pm.MAT_FRESNEL if m["kind"] == "fresnel" else pm.MAT_PHONG for m in mt])
    lkind = np.array([pm.LIGHT_POINT if s.lights[0]["kind"] == "point" else pm.LIGHT_DIRECTIONAL for s in specs])
    lv = col(lambda s: s.lights[0].get("location", s.lights[0].get("direction")))
    lc = col(lambda s: s.lights[0]["color"])
    bg = np.tile(np.array(specs[0].background), (n, 1))

    hit = pm.sphere(o, d, c, r)
    assert hit["hit"].all()
    s = pm.shade(hit["pt"], hit["n"], d, kd, ks, exponent, ior, mat, lkind, lv, lc, np.ones(n))
    trivial = exponent <= 1.0
    libm_p = np.array([math.pow(a, b) for a, b in zip(s["c"], exponent)])
    assert pm.bits_equal(s["p"][trivial], libm_p[trivial]).all()
    s["p"] = libm_p
    shadow = pm.sphere(hit["pt"] + s["ldir"] * pm.K_EPS, s["ldir"], c, r)                    # raytrace.rs:41-49
    shadowed = shadow["hit"] & (~s["has_range"] | (shadow["t"] * shadow["t"] < s["r2"]))
    lit = (s["diffuse"] | s["specular"]) & ~shadowed
    res = pm.add_light(amb, kd, ks, lc, s["f"], s["ldir"], s["n"], s["p"], s["diffuse"] & lit, s["specular"] & lit)
    mirror = pm.sphere(s["refl"][:, :3], s["refl"][:, 3:], c, r)
    assert not mirror["hit"].any()                         # a convex object: the mirror ray sees the background
    res = np.where(s["specular"][:, None], res + (ks * bg) * s["f"][:, None], res)             # raytrace.rs:63 / 163
    # every class the docstring names is there
    back = pm.dot(s["ldir"], s["n"]) < 0.0
    for e in (0.0, 1.0, 32.0, 2.5):
        for k in (pm.MAT_PHONG, pm.MAT_FRESNEL):
            for lk in (pm.LIGHT_POINT, pm.LIGHT_DIRECTIONAL):
                sel = (exponent == e) & (mat == k) & (lkind == lk)
                assert (sel & lit).sum() >= 3 and (sel & back).sum() >= 1, (e, k, lk)
    assert shadowed.sum() >= 40 and (~s["specular"] & s["diffuse"]).sum() >= 20 and (lit & s["specular"]).sum() >= 100
    for i, spec in enumerate(specs):
        ref = ref64.render(spec)["rgb64"][0, 0]
        assert pm.bits_equal(res[i], ref).all(), (i, spec.name, res[i], ref, lit[i], mat[i], exponent[i])


# ---- the correctly rounded libm fixture ------------------------------------------------------------------
def _fixture():
    sys.path.insert(0, GOLDEN)
    import make_libm_fixtures as mk
    z = np.load(os.path.join(GOLDEN, "libm_cr.npz"))
    n = int(z["n"])
    assert n == pm.N_FIXTURE and int(z["prec"]) >= 200
    c, y = pm.pow_operands(n)
    x = pm.trig_operands(n)
    assert [mk.crc(c), mk.crc(y), mk.crc(x)] == list(z["operands_crc"]), "prim_model.py no longer forms the fixture's operands"
    return mk, z, {"pow": (c, y), "sin": (x,), "cos": (x,)}


def test_libm_fixture_operands_and_the_host_libm_beside_it():
    """libm_cr.npz belongs to the operands prim_model.py forms (their checksums), and the host libm lies within
    one representable value of it everywhere (glibc documents < 1 ulp for pow, sin and cos); how many of its
    results differ at all is printed."""
    _, z, ops = _fixture()
    for fn, a in ops.items():
        with np.errstate(all="ignore"):
            host = {"pow": np.power, "sin": np.sin, "cos": np.cos}[fn](*a)
        dist = pm.low16_distance(host, z[fn + "_low16"])
        print(f"host {fn}: {np.count_nonzero(dist)} of {len(dist)} differ from correctly rounded, largest distance {np.abs(dist).max()}")
        assert np.abs(dist).max() <= 1, fn


def test_libm_fixture_recomputed():
    """A sample of 600 results per function, and the 24 operands nearest the multiples of pi / 4, recomputed
    with mpmath at 200 bits, have the recorded low ordinal bits; and the host libm lies within one
    representable value of the recomputed values in full, so its distance read from the low bits above is
    its distance."""
    import mpmath  # noqa: F401  (make_libm_fixtures needs it: a missing module fails this test)
    mk, z, ops = _fixture()
    n = int(z["n"])
    idx = np.union1d(np.random.default_rng(3).choice(n, 600, replace=False), np.arange(n - 24, n))
    for fn, a in ops.items():
        cr = mk.correctly_rounded(fn, *[v[idx] for v in a])
        assert np.array_equal(mk.low16(cr), z[fn + "_low16"][idx]), fn
        with np.errstate(all="ignore"):
            host = {"pow": np.power, "sin": np.sin, "cos": np.cos}[fn](*[v[idx] for v in a])
        assert np.abs(pm.ordinal(host) - pm.ordinal(cr)).max() <= 1, fn
