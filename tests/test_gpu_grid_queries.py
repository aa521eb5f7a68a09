"""The grid queries on staged scene constants.

The grid sources (wf_occlusion<14 / 15>, the camera pass wf_nearest<22 / 23>) keep the lights, every
light's grid header (per-face fields re-packed) and the planes in LDS, request a cell's offsets before
the own-sphere test, and load list entry e + 1 before entry e is tested.  None of that may change a
test or a stop, so every case here is compared with the oracle as tests/test_gpu_fold_levels.py does
(BGR bytes equal, f32 within 1e-5 relative, rays and shadow rays equal; the oracle's renders computed
once per scene and left unchanged), and its four RT_COUNT_WORK counters with
tests/golden/grid_query_counts.json, recorded from the library of the commit before the change: equal
counters are the proof that the same spheres are still tested.

The cases are the smallest at which the new code can go wrong.  Frames of 64x48 (whole 8x8 tiles) and
61x45 (partial tiles; a generation's record count is then no multiple of 64, so one wave's lanes
carry two different lights and index two headers):
  * 1, 3 and 5 point lights on config3's geometry, and the 3-light scene with a directional light
    second in the list (no grid for it: the general shadow kernel answers the point lights through
    the grids in L2, next to the staged camera pass);
  * a ground plane (staged planes on the shadow and the camera path);
  * grids forced to 16 cells per side (few, long lists) and 512 (empty and one-entry lists), for
    the lights and for the camera;
  * lights inside a sphere's padded box (a non-empty always list: test_lightgrid.py's light set);
  * every route the planner offers: grid_occ 1 / 0 and cam 3 / 0 by tuning, and a 2500-sphere scene
    whose sphere list is beyond LDS, where the planner itself takes the G variants (grid_occ 2,
    cam 4: they are plan results, not tuning values);
  * the fused tail from generations 1 and 4 (grid_shadow_mask).

Regenerate the counters (only when a grid query changes its tests on purpose):
    python tests/test_gpu_grid_queries.py OUT.json
"""
import contextlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "rust-raytrace_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import libraytrace as lr  # noqa: E402
from libraytrace import scenes  # noqa: E402
from oracle import ref64  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "grid_query_counts.json")
FIELDS = ("box_tests", "sphere_tests", "shadow_box_tests", "shadow_sphere_tests")
RTOL = 1e-5
F32_SUBNORMAL_HALF_STEP = 2.0 ** -150
WF = lr.RT_ALGO_WAVEFRONT
SIZES = {"64x48": (64, 48), "61x45": (61, 45)}

POINT_LIGHTS = [((-10.0, 10.0, 5.0), (0.8, 0.8, 0.8)), ((10.0, 8.0, 0.0), (0.6, 0.6, 0.6)),
                ((0.0, 12.0, -8.0), (0.4, 0.4, 0.5)), ((-6.0, 3.0, 8.0), (0.3, 0.2, 0.2)),
                ((7.0, 1.0, 6.0), (0.2, 0.3, 0.2))]


def _c3_lights(n_point, directional_second=False):
    def make(w, h):
        s = scenes.config3(w, h)
        s.lights = []
        for k, (loc, col) in enumerate(POINT_LIGHTS[:n_point]):
            if k == 1 and directional_second:
                s.directional_light((0.2, -1.0, -0.1), (0.2, 0.2, 0.2))
            s.point_light(loc, col)
        return s
    return make


def _adversarial(w, h):
    """test_lightgrid.py's spheres and lights: a light at a sphere's centre and one on its surface."""
    s = scenes.SceneSpec(width=w, height=h, max_depth=4, background=(0.05, 0.05, 0.1),
                         camera={"ctor": "new", "position": (0, 2, 12), "look": (0, -0.1, -1), "up": (0, 1, 0),
                                 "im_dist": 1.2})
    rng = scenes.SplitMix64(4242)
    for _ in range(400):
        cen = (rng.uniform(-6, 6), rng.uniform(-2, 6), rng.uniform(-10, 2))
        kd = (rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9))
        s.sphere(cen, 10 ** rng.uniform(-3, -0.2), scenes.phong(kd, (0.3, 0.3, 0.3), 20.0, (0.01, 0.01, 0.01)))
    s.sphere((3.0, 1.0, -4.0), 0.8, scenes.phong((0.8, 0.8, 0.2), (0.4, 0.4, 0.4), 10.0, (0, 0, 0)))
    s.sphere((0.0, -1e3 - 2.5, -4.0), 1e3, scenes.phong((0.5, 0.5, 0.5), (0.2, 0.2, 0.2), 5.0, (0, 0, 0)))
    s.point_light((0.0, 2.0, -4.0), (0.6, 0.6, 0.6))
    s.point_light((3.0, 1.0, -4.0), (0.5, 0.2, 0.2))
    s.point_light((3.0, 1.8, -4.0), (0.2, 0.5, 0.2))
    s.point_light((-5.0, 0.5, -30.0), (0.2, 0.2, 0.5))
    return s


SCENES = {
    "lights1": _c3_lights(1),
    "lights3": _c3_lights(3),
    "lights5": _c3_lights(5),
    "lights3_dir": _c3_lights(3, directional_second=True),
    "planes": lambda w, h: scenes.random_spheres(200, w, h, 4, seed=21, name="gq_planes", plane=True),
    "always": _adversarial,
    "big": lambda w, h: scenes.random_spheres(2500, w, h, 4, seed=12, box_scale=2.0, name="gq_big"),
}

# name -> (scene, size, tuning)
CASES = {}
for _sc in ("lights1", "lights3", "lights5", "lights3_dir", "planes", "always"):
    for _sz in SIZES:
        CASES[f"{_sc}_{_sz}"] = (_sc, _sz, {})
for _res in (16, 512):
    CASES[f"lights3_lgrid{_res}"] = ("lights3", "61x45", dict(light_grid_res=_res))
    CASES[f"lights3_cgrid{_res}"] = ("lights3", "61x45", dict(cam_grid_res=_res))
for _sc in ("lights3", "planes"):
    for _occ in (1, 0):
        for _cam in (3, 0):
            CASES[f"{_sc}_gridocc{_occ}_cam{_cam}"] = (_sc, "61x45", dict(grid_occ=_occ, cam=_cam))
CASES["big_61x45"] = ("big", "61x45", {})                        # the planner: grid_occ 2, cam 4
CASES["big_cam0"] = ("big", "61x45", dict(cam=0))
for _t in (1, 4):
    CASES[f"lights3_tail{_t}"] = ("lights3", "61x45", dict(tail_fuse=_t))

_refs = {}


def oracle(scene, size):
    if (scene, size) not in _refs:
        _refs[(scene, size)] = ref64.render(SCENES[scene](*SIZES[size]),
                                            threads=min(16, os.cpu_count() or 1) if scene == "big" else 1)
    return _refs[(scene, size)]


@contextlib.contextmanager
def tuning(ctx, **kv):
    old = {k: ctx.get_tuning(k) for k in kv}
    try:
        for k, v in kv.items():
            ctx.set_tuning(k, v)
        yield
    finally:
        for k, v in old.items():
            ctx.set_tuning(k, v)


def render_case(ctx, name, flags=0):
    """(rgb, bgr, stats, shade records per generation) of one case; the grid resolutions take effect at upload."""
    scene, size, tune = CASES[name]
    spec = SCENES[scene](*SIZES[size])
    with tuning(ctx, **tune):
        ctx.upload(lr.Scene.deserialize(spec.to_text()))
        o = lr.render_opts(spec.width, spec.height, max_depth=spec.max_depth, spp=1, algo=WF,
                           flags=lr.RT_OUT_RGB_F32 | lr.RT_OUT_BGR_U8 | flags)
        rgb, bgr, st = ctx.render(o)
        records = ctx.generation_counts()[1]
    return rgb, bgr, st, records


def assert_f32(rgb, r64):
    g = rgb.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        r32 = r64.astype(np.float32).astype(np.float64)
        ok = ((np.isnan(r64) & np.isnan(g)) | (np.isinf(r32) & (r32 == g)) |
              (np.abs(g - r64) <= RTOL * np.abs(r64) + F32_SUBNORMAL_HALF_STEP))
    assert ok.all(), f"{(~ok).sum()} colour components beyond rtol {RTOL}"


def test_fixture_covers_the_cases():
    with open(FIXTURE) as f:
        want = json.load(f)
    assert set(want) == set(CASES)
    # a forced resolution changes the lists walked: the counters see it (coarse cells, longer lists)
    assert want["lights3_lgrid16"][3] > want["lights3_61x45"][3] > want["lights3_lgrid512"][3]
    assert want["lights3_cgrid16"][1] - want["lights3_cgrid16"][3] > want["lights3_cgrid512"][1] - want["lights3_cgrid512"][3]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_grid_query_case(gpu_ctx, name):
    scene, size, _ = CASES[name]
    ref = oracle(scene, size)
    rgb, bgr, st, records = render_case(gpu_ctx, name)
    assert np.array_equal(bgr, ref["bgr"]), f"{(bgr != ref['bgr']).sum()} BGR bytes differ"
    assert_f32(rgb, ref["rgb64"])
    assert (st.rays, st.shadow_rays) == (ref["counts"]["rays"], ref["counts"]["shadow_rays"])
    if size == "61x45":
        # a wave of the shadow kernel then holds the last records of light l and the first of l + 1
        assert any(r % 64 for r in records), records
    with open(FIXTURE) as f:
        want = json.load(f)[name]
    got = [int(getattr(render_case(gpu_ctx, name, lr.RT_COUNT_WORK)[2], f)) for f in FIELDS]
    print(name, dict(zip(FIELDS, got)))
    assert got == want


if __name__ == "__main__":
    with lr.Context(0) as _ctx:
        _got = {_n: [int(getattr(render_case(_ctx, _n, lr.RT_COUNT_WORK)[2], _f)) for _f in FIELDS] for _n in CASES}
    with open(sys.argv[1], "w") as _f:
        json.dump(_got, _f, indent=1)
        _f.write("\n")
    for _k, _v in _got.items():
        print(_k, _v)
