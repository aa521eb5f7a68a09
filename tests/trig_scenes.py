"""The scenes whose random draws go through cos / sin (IndirectPhong bounce
directions, raytrace.rs:104-105; the DoF lens offset, camera.rs:119), and the
perturbation envelope they are judged by.

glibc and the device's libm may differ in the last ulp of cos, sin and pow.  How
far that can move an image is measured on the reference alone: the oracle renders
each scene with every material / camera cos, sin and pow result moved by
k in PERTURBATIONS (ref_opts.trig_ulps).  A BGR byte that is the same in all of
those renders is *stable*: no last-ulp difference of a libm reaches it, so the
device must produce it exactly.  tests/test_oracle_trig.py (CPU) requires of every
scene here that the ray counts and NaN masks do not move at all and that at least
STABLE_MIN of the bytes are stable; tests/test_gpu_path.py then holds the device to
the counts, the NaN mask, every stable byte, and to one of the envelope's values
on the rest.
"""
import functools

import numpy as np

from libraytrace import scenes
from oracle import ref64
from cornell import cornell_spec

# (trig_ulps, trig_hashed): libm's own results first, then uniform +-1, +-4 and the hashed +-1
PERTURBATIONS = [(0, False), (1, False), (-1, False), (4, False), (-4, False), (1, True), (-1, True)]
STABLE_MIN = 0.9999


def stochastic_dof():
    """IndirectPhong x2 samples, DoF x2 lens samples, AreaLight, Transparent; seed 3."""
    return scenes.stochastic(96, 64, antialias=4, samples=2, dof=True)


def cornell_small():
    return cornell_spec(64, 64, antialias=16)


def edge_scene():
    """Reference quirks and corner cases of the stochastic / branching classes."""
    spec = scenes.SceneSpec(width=72, height=48, antialias=2, max_depth=3, camera=dict(scenes.DEFAULT_CAMERA),
                            background=(0.3, 0.2, 0.1))
    # IndirectPhong with ks > 0: the specular term is pow(NaN, exp) (raytrace.rs:108,115) -> NaN pixels
    spec.sphere((-2.0, 1.0, -6.0), 1.0, scenes.indirect_phong((0.5, 0.5, 0.5), (0.2, 0.2, 0.2), 8.0, (0.0,) * 3, 1))
    # IndirectPhong with samples = 0: direct light only, no bounce
    spec.sphere((0.0, 1.0, -6.0), 1.0, scenes.indirect_phong((0.4, 0.6, 0.2), (0.0,) * 3, 1.0, (0.01,) * 3, 0))
    # dense glass: total internal reflection inside (refract None -> fresnel 1)
    spec.sphere((2.0, 1.0, -6.0), 1.0, scenes.transparent((1.0, 1.0, 1.0), 32.0, 2.4))
    spec.plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), scenes.phong((0.5, 0.5, 0.5), (0.3,) * 3, 16.0, (0.01,) * 3))
    spec.area_light((-1.0, 6.0, -4.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5))   # degenerate: a point
    spec.area_light((2.0, 7.0, -3.0), (1.5, 0.0, 0.0), (0.0, 0.0, 1.5), (0.4, 0.4, 0.4))
    spec.directional_light((0.0, -1.0, -0.5), (0.2, 0.2, 0.2))
    return spec


def dof_config2(aperture=0.3, samples=3):
    spec = scenes.config2(64, 36)
    spec.depth_of_field(6.0, aperture, samples)
    return spec


def convex_bounce(samples, max_depth, specular=False):
    """One IndirectPhong sphere on an IndirectPhong plane under a point and an area
    light: every hit spawns `samples` bounce rays, each keyed child(K, i), and a
    frame with samples > 1 stores and reloads its extension between them.
    specular: ks > 0 with exponent 0 -- the bounce's specular factor is pow(NaN, 0),
    which is 1 (C99 / IEEE 754 pow), so the specular fold carries finite colours."""
    ks, ex = ((0.25, 0.2, 0.15), 0.0) if specular else ((0.0, 0.0, 0.0), 1.0)
    spec = scenes.SceneSpec(width=64, height=48, antialias=1, max_depth=max_depth, camera=dict(scenes.DEFAULT_CAMERA),
                            background=(0.25, 0.3, 0.4))
    spec.sphere((0.3, 1.4, -6.0), 1.4, scenes.indirect_phong((0.7, 0.4, 0.3), ks, ex, (0.02, 0.01, 0.0), samples))
    spec.plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), scenes.indirect_phong((0.5, 0.55, 0.6), ks, ex, (0.01,) * 3, samples))
    spec.point_light((-6.0, 9.0, 3.0), (0.7, 0.7, 0.7))
    spec.area_light((3.0, 8.0, -2.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (0.6, 0.55, 0.5))
    return spec


CONVEX_CASES = [(s, d) for s in (1, 2, 5) for d in (1, 3)]

# name -> (builder, seed, jitter): every trig scene the GPU tests render
TRIG_SCENES = {
    "stochastic_dof": (stochastic_dof, 3, 1),
    "cornell_64x64x16": (cornell_small, 1, 1),
    "edge_scene": (edge_scene, 32, 1),
    "dof_config2": (dof_config2, 7, 1),
    "convex_specular_exp0": (lambda: convex_bounce(2, 2, specular=True), 41, 1),
}
for _s, _d in CONVEX_CASES:
    TRIG_SCENES[f"convex_s{_s}_d{_d}"] = (functools.partial(convex_bounce, _s, _d), 40, 1)


class Envelope:
    """The oracle's renders of one scene under PERTURBATIONS."""

    def __init__(self, spec, seed, jitter):
        self.renders = [ref64.render(spec, jitter=jitter, seed=seed, rng=1, trig_ulps=k, trig_hashed=h)
                        for k, h in PERTURBATIONS]
        self.ref = self.renders[0]
        bgrs = np.stack([r["bgr"] for r in self.renders])
        self.bgrs = bgrs
        self.stable = (bgrs == bgrs[0]).all(axis=0)
        self.stable_share = float(self.stable.mean())
        self.nan = np.isnan(self.ref["rgb64"])
        self.counts_equal = all(r["counts"]["rays"] == self.ref["counts"]["rays"] and
                                r["counts"]["shadow_rays"] == self.ref["counts"]["shadow_rays"] for r in self.renders)
        self.nan_equal = all(np.array_equal(np.isnan(r["rgb64"]), self.nan) for r in self.renders)
        fin = ~self.nan
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = [np.abs(r["rgb64"][fin] - self.ref["rgb64"][fin]) / np.abs(self.ref["rgb64"][fin]) for r in self.renders]
        self.max_rel = float(max((np.nanmax(x) if x.size else 0.0) for x in rel))

    def check_scene(self):
        """What a trig scene (geometry and seed) has to satisfy before a device is judged by it."""
        assert self.counts_equal, "a last-ulp change of cos / sin / pow changes what a ray hits: pick another seed"
        assert self.nan_equal, "a last-ulp change of cos / sin / pow moves the NaN pixels"
        assert self.stable_share >= STABLE_MIN, f"only {self.stable_share:.6f} of the BGR bytes are stable"


_cache = {}


def envelope(spec, seed, jitter=1):
    key = (spec.to_text(), spec.max_depth, seed, jitter)
    if key not in _cache:
        _cache[key] = Envelope(spec, seed, jitter)
    return _cache[key]
