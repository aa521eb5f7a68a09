"""The sphere source asked for is the source that runs.

Every sphere source of the wavefront schedule gives the same pixels and the same ray counts, so
the parity tests cannot tell whether launch_wavefront sent source 8 to source 5's kernel.  The work
counters can: RT_COUNT_WORK counts the box and sphere tests of the nearest-hit and of the shadow
queries, and they depend on the structure walked.  One small frame is rendered once per (src,
src_occ) pair of launch_wavefront and once per camera / shadow-grid route, and the four counters
are compared with tests/golden/source_counts.json, recorded from the library as it was before the
kernels were split over several translation units (commit 864830e).

Two scenes, because the planner offers a pair only where it applies: 200 spheres (tree and
spheres fit LDS: sources 1, 2, 7, 9, 8, 25, 26 and the grids) and 2500 spheres (a sphere list and
a tree beyond LDS: the brute-force source 0 and the binary16 prefix sources 5 and 6).

Regenerate (only when a traversal changes on purpose): python tests/test_gpu_sources.py OUT.json
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "rust-raytrace_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import libraytrace as lr  # noqa: E402
from libraytrace import scenes  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "source_counts.json")
FIELDS = ("box_tests", "sphere_tests", "shadow_box_tests", "shadow_sphere_tests")

SCENES = {
    "small": lambda: scenes.random_spheres(200, 64, 48, 4, seed=11, name="sources"),
    "big": lambda: scenes.random_spheres(2500, 64, 48, 4, seed=12, box_scale=2.0, name="sources_big"),
}

# The pairs walk their own structures only without the light-view grids (with them every shadow
# query of a point light goes through its grid, whatever src_occ says) and without the camera's
# view grid (which would take generation 0).  Sources 5, 6, 8 and 26 get a 1 KB LDS prefix, so
# that most of the tree is below it.
_PAIR = dict(light_grids=0, cam=0)
W, B = lr.RT_ALGO_WAVEFRONT, lr.RT_ALGO_WAVEFRONT_BRUTE
CONFIGS = {
    "1_1": ("small", B, dict(_PAIR)),
    "2_2": ("small", W, dict(_PAIR, src=2, src_occ=2)),
    "7_7": ("small", W, dict(_PAIR, src=7, src_occ=7)),
    "7_10": ("small", W, dict(_PAIR, src=7, src_occ=10)),
    "9_10": ("small", W, dict(_PAIR, src=9, src_occ=10)),
    "2_11": ("small", W, dict(_PAIR, src=2, src_occ=11)),
    "8_11": ("small", W, dict(_PAIR, src=8, src_occ=11, prefix_kb=1)),
    "25_11": ("small", W, dict(_PAIR, src=25, src_occ=11)),
    "26_11": ("small", W, dict(_PAIR, src=26, src_occ=11, prefix_kb=1)),
    # the default sources with the grids: the camera's view grid or not, the shadow kernel
    # without a tree walk or the general one
    "cam3_gridocc1": ("small", W, dict(cam=3, grid_occ=1)),
    "cam0_gridocc1": ("small", W, dict(cam=0, grid_occ=1)),
    "cam3_gridocc0": ("small", W, dict(cam=3, grid_occ=0)),
    "big_0_0": ("big", B, dict(_PAIR)),
    "big_2_11": ("big", W, dict(_PAIR, src=2, src_occ=11)),
    "big_5_11": ("big", W, dict(_PAIR, src=5, src_occ=11, prefix_kb=1)),
    "big_6_11": ("big", W, dict(_PAIR, src=6, src_occ=11, prefix_kb=1)),
    "big_8_11": ("big", W, dict(_PAIR, src=8, src_occ=11, prefix_kb=1)),
}

# (box, sphere) tests of the nearest-hit queries alone: the counters hold both kinds of query
def _nearest(v):
    return (v[0] - v[2], v[1] - v[3])


def _shadow(v):
    return (v[2], v[3])


# Structures the counters must tell apart: brute force, the binary tree with 64-bit and with
# compact stack entries (7 and 9, 5 and 6: the compact entry keeps fewer bits of the entry
# distance, and the walks differ by a few node visits), the quantised 4-wide tree, the camera grid; on the big scene
# brute force, the f32 tree and the binary16 tree.  For the shadow queries: brute force, the
# binary tree, the 4-wide tree, the light grids.
DISTINCT_NEAREST = [("1_1", "7_7", "9_10", "25_11", "cam3_gridocc1"), ("big_0_0", "big_2_11", "big_5_11", "big_6_11")]
DISTINCT_SHADOW = [("1_1", "7_7", "7_10", "cam3_gridocc1")]
# Configurations that walk identically by design, named here because their counters cannot tell
# them apart (the kernel names of a profiler's trace do):
#   2, 7 and 8: the same binary tree and the same walk, read from HBM/L2, LDS or an LDS prefix
#   25 and 26: the same quantised tree, whole in LDS or an LDS prefix
#   10 and 11: the same 4-wide tree, in LDS or through L2
#   grid_occ 0 and 1: with a grid for every light both shadow kernels answer through the grids
SAME_NEAREST = [("2_2", "2_11", "7_7", "7_10", "8_11"), ("25_11", "26_11"), ("big_2_11", "big_8_11")]
SAME_SHADOW = [("7_10", "9_10", "2_11", "8_11", "25_11", "26_11"), ("2_2", "7_7"),
               ("cam3_gridocc1", "cam0_gridocc1", "cam3_gridocc0"), ("big_2_11", "big_5_11", "big_6_11", "big_8_11")]


def measure(ctx, only=None):
    """{config: [box_tests, sphere_tests, shadow_box_tests, shadow_sphere_tests]}"""
    out = {}
    for name, (scene, algo, tuning) in CONFIGS.items():
        if only and name not in only:
            continue
        spec = SCENES[scene]()
        old = {k: ctx.get_tuning(k) for k in tuning}
        try:
            for k, v in tuning.items():
                ctx.set_tuning(k, v)
            ctx.upload(lr.Scene.deserialize(spec.to_text()))          # (light_grids takes effect at upload)
            o = lr.render_opts(spec.width, spec.height, max_depth=spec.max_depth, spp=1, algo=algo,
                               flags=lr.RT_OUT_RGB_F32 | lr.RT_OUT_BGR_U8 | lr.RT_COUNT_WORK)
            st = ctx.render(o)[2]
        finally:
            for k, v in old.items():
                ctx.set_tuning(k, v)
        out[name] = [int(getattr(st, f)) for f in FIELDS]
    return out


def test_fixture_tells_the_structures_apart():
    """The recorded counters differ wherever the traversals differ in structure, and are equal
    only where the walks are the same by design."""
    with open(FIXTURE) as f:
        want = json.load(f)
    assert set(want) == set(CONFIGS)
    for part, distinct, same in ((_nearest, DISTINCT_NEAREST, SAME_NEAREST), (_shadow, DISTINCT_SHADOW, SAME_SHADOW)):
        for group in distinct:
            assert len({part(want[k]) for k in group}) == len(group), (part.__name__, group)
        for group in same:
            assert len({part(want[k]) for k in group}) == 1, (part.__name__, group)


@pytest.mark.gpu
def test_every_source_runs_its_own_kernel(gpu_ctx):
    with open(FIXTURE) as f:
        want = json.load(f)
    got = measure(gpu_ctx)
    for name in CONFIGS:
        print(name, dict(zip(FIELDS, got[name])))
    assert got == want


if __name__ == "__main__":
    with lr.Context(0) as _ctx:
        _got = measure(_ctx)
    with open(sys.argv[1], "w") as _f:
        json.dump(_got, _f, indent=1)
        _f.write("\n")
    for _k, _v in _got.items():
        print(_k, _v, _nearest(_v))
