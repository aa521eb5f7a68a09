"""Adversarial scenes shared by the wavefront parity tests (test_gpu_parity.py) and
the path kernel's (test_gpu_path.py): NaN plane hits, coincident objects,
exact-axis rays and ties across BVH leaves, operands far from unit magnitude."""
from libraytrace import scenes


def tiny(**kw):
    s = scenes.SceneSpec(width=kw.pop("width", 8), height=kw.pop("height", 8), max_depth=kw.pop("max_depth", 4),
                         background=(0.2, 0.3, 0.4),
                         camera={"ctor": "new", "position": (0, 0, 0), "look": (0, 0, -1), "up": (0, 1, 0),
                                 "im_dist": 1.0})
    return s


def nan_plane_scene():
    """test_nan_plane_wins's camera-in-a-plane scene (NaN plane hits) with 60
    more spheres, so that the wave query has several clusters to cull."""
    s = tiny(width=17, height=13)
    s.max_depth = 5
    s.sphere((0, 0, -5), 1.0, scenes.phong((0.5, 0.5, 0.5), (0.3, 0.3, 0.3), 8.0, (0, 1, 0)))
    rng = scenes.SplitMix64(21)
    for k in range(60):
        c = (rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(-12, -3))
        s.sphere(c, rng.uniform(0.1, 0.8), scenes.phong((0.4, 0.5, 0.6), (0.5, 0.5, 0.5), 20.0, (0, 0, 0)))
    s.plane((0, 0, 0), (0, 1, 0), scenes.phong((0.1, 0.2, 0.3), (0.2, 0.2, 0.2), 4.0, (0, 0, 1)))
    s.point_light((3, 3, 3), (1, 1, 1))
    s.directional_light((0, -1, 0.2), (0.5, 0.5, 0.5))
    return s


def axis_tie_scene():
    s = scenes.SceneSpec(width=33, height=31, max_depth=6, background=(0.1, 0.1, 0.2),
                         camera={"ctor": "new", "position": (0, 0, 0), "look": (0, 0, -1), "up": (0, 1, 0),
                                 "im_dist": 1.0})
    rng = scenes.SplitMix64(77)
    for k in range(24):
        kd = (rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0, 1))
        s.sphere((0.0, 0.0, -6.0), 1.5, scenes.phong(kd, (0.3, 0.3, 0.3), 20.0, (0.01, 0.01, 0.01)))
    for k in range(300):     # clutter so the duplicates spread over the tree
        c = (rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(-20, -3))
        s.sphere(c, rng.uniform(0.05, 0.5), scenes.phong((0.5, 0.5, 0.5), (0.4, 0.4, 0.4), 30.0, (0, 0, 0)))
    # spheres exactly tangent to the axis rays and to each other
    s.sphere((1.0, 0.0, -10.0), 1.0, scenes.phong((0.9, 0.2, 0.2), (0.5, 0.5, 0.5), 8.0, (0, 0, 0)))
    s.sphere((-1.0, 0.0, -10.0), 1.0, scenes.phong((0.2, 0.9, 0.2), (0.5, 0.5, 0.5), 8.0, (0, 0, 0)))
    s.point_light((0.0, 5.0, 0.0), (1, 1, 1))
    s.directional_light((0.0, -1.0, 0.0), (0.3, 0.3, 0.3))
    return s


def coincident_scene():
    """Two spheres and two planes at the same place: the first in file order wins (scene.rs:223-249)."""
    s = tiny(width=16, height=16)
    a = scenes.phong((0.9, 0.1, 0.1), (0.2, 0.2, 0.2), 10.0, (0.1, 0, 0))
    b = scenes.phong((0.1, 0.9, 0.1), (0.2, 0.2, 0.2), 10.0, (0, 0.1, 0))
    s.sphere((0.3, 0, -4), 1.0, a)
    s.sphere((0.3, 0, -4), 1.0, b)
    s.plane((0, -1, 0), (0, 1, 0), a)
    s.plane((0, -1, 0), (0, 1, 0), b)
    s.point_light((2, 3, 0), (1, 1, 1))
    return s


def extreme_magnitudes_scene():
    """A directional light of magnitude 1e-35 (its shadow rays keep the unnormalised
    -direction, a = 1e-70), one of magnitude 1e34, and mirror planes with normals of
    length 1e25 and 1e-20 (reflection directions d - 2n(d.n) far from unit length),
    over random spheres."""
    s = scenes.random_spheres(60, 64, 48, 6, seed=33, plane=False)
    s.lights = []
    s.directional_light((3e-36, -1e-35, -2e-36), (0.5, 0.5, 0.4))
    s.directional_light((2e33, -1e34, 1e33), (0.0, 0.0, 0.0))       # (black: its shadow rays still run)
    s.point_light((0.0, 8.0, 2.0), (0.6, 0.6, 0.6))
    s.plane((0.0, -0.5, 0.0), (0.0, 1e25, 0.0), scenes.phong((0.2, 0.2, 0.2), (0.6, 0.6, 0.6), 10.0, (0.01, 0.01, 0.01)))
    s.plane((0.0, 0.0, -40.0), (0.0, 3e-21, 1e-20), scenes.phong((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 10.0, (0.0, 0.0, 0.0)))
    return s
