"""Scenes whose pixels are exactly chosen f64 values: every sRGB threshold T_i and the value just below it, as
the colour of at least one pixel, by three routes that end in three different pixel writers (DESIGN.md §4,
"Output stage").  A helper of test_output_model.py (which asserts on the oracle's output that the values
really arrive, exactly, on every route) and of test_gpu_output.py.

170 spheres of radius 0.4 on a 17 x 10 lattice, one triple of the 510 values each as (r, g, b):
  A  ambient end: the spheres are phong(kd 0, ks 0, exponent 1, ambient v), so the camera ray's chain ends at
     the hit and the pixel is v, written by whatever finishes the camera pass.
  B  a lit record that adds zero: phong(kd 1, ks 0, 1, ambient v) under a point light of colour (0, 0, 0): the
     camera hit becomes a shade record and a chain of no levels, and the fold (or the fused tail) emits v + 0.
  C  one fold level: a mirror plane phong(kd 0, ks 1, 1, ambient 0) fills the view and reflects route A's
     spheres, which stand behind the camera: every pixel is a chain of one level, 0 + (1 v) 1 or the
     reflected background.
The distance camera -> (mirror ->) lattice is 12 on every route, so the three frames show the same lattice.
No pow result survives in any of them (the light's colour is zero), so the device's f32 output must equal
the oracle's bit for bit.
"""
import numpy as np

from libraytrace import scenes

import output_model as om

WIDTH, HEIGHT = 340, 200
COLS, ROWS, RADIUS = 17, 10, 0.4
BACKGROUND = (0.3, 0.2, 0.1)                  # no threshold, no neighbour of one
ROUTES = ("A", "B", "C")
CAMERA = {"ctor": "new", "position": (0.0, 2.0, 10.0), "look": (0.0, 0.0, -1.0), "up": (0.0, 1.0, 0.0), "im_dist": 1.5}


def triples():
    """[170, 3]: the 510 values T_0, below(T_0), T_1, ... dealt three to a sphere."""
    return om.threshold_values().reshape(170, 3)


def scene(route, spp=1):
    s = scenes.SceneSpec(width=WIDTH, height=HEIGHT, antialias=spp, max_depth=4, name="thr" + route,
                         camera=dict(CAMERA), background=BACKGROUND)
    z = -2.0 if route != "C" else 14.0        # C: behind the camera, 4 + 8 from it by way of the mirror at z = 6
    for k, v in enumerate(triples()):
        c = ((k % COLS) - (COLS - 1) / 2.0, 2.0 + ((k // COLS) - (ROWS - 1) / 2.0), z)
        kd = (1.0, 1.0, 1.0) if route == "B" else (0.0, 0.0, 0.0)
        s.sphere(c, RADIUS, scenes.phong(kd, (0.0, 0.0, 0.0), 1.0, tuple(float(x) for x in v)))
    if route == "C":
        s.plane((0.0, 0.0, 6.0), (0.0, 0.0, 1.0), scenes.phong((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1.0, (0.0, 0.0, 0.0)))
    s.point_light((3.0, 9.0, 8.0), (0.0, 0.0, 0.0))
    return s


def background_scenes():
    """Eight one-sphere scenes (16 x 12) whose BACKGROUND is a threshold triple -- T_0, T_254 and their lower
    neighbours among them: the pixels the host computes (bg_rgb, bg_bgr)."""
    t = om.threshold_values()
    picks = [(t[0, 0], t[0, 1], t[254, 0]), (t[254, 1], t[254, 0], t[0, 1]), (t[1, 1], t[127, 0], t[127, 1]),
             (t[253, 0], t[253, 1], t[1, 0]), (t[64, 0], t[64, 1], t[200, 1]), (t[200, 0], t[31, 1], t[31, 0]),
             (t[0, 0], t[0, 0], t[0, 0]), (t[254, 1], t[254, 1], t[254, 1])]
    out = []
    for bg in picks:
        s = scenes.SceneSpec(width=16, height=12, antialias=1, max_depth=2, name="thrbg", camera=dict(CAMERA),
                             background=tuple(float(x) for x in bg))
        s.sphere((0.0, 2.0, -2.0), 1.0, scenes.phong((0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 1.0, (0.01, 0.02, 0.03)))
        s.point_light((3.0, 9.0, 8.0), (0.5, 0.5, 0.5))
        out.append(s)
    return out


def pixels_per_triple(rgb64):
    """[170]: the pixels of an oracle frame [h, w, 3] whose f64 colour is, bit for bit, sphere k's triple."""
    px = np.ascontiguousarray(rgb64).view(np.uint64).reshape(-1, 3)
    return np.array([(px == np.ascontiguousarray(v).view(np.uint64)).all(axis=1).sum() for v in triples()])


def values_present(rgb64, channels_of=None):
    """[255, 2] bool: which of the 510 values occur, bit for bit, among the f64 colour components of an
    oracle frame (channels_of: a bool mask [h, w] restricting the pixels)."""
    a = rgb64 if channels_of is None else rgb64[channels_of]
    have = np.unique(np.ascontiguousarray(a).view(np.uint64))
    return np.isin(om.threshold_values().view(np.uint64), have)
