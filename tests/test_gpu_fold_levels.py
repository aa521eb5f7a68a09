"""The packed level entries of the wavefront schedules (WfLevel).

A level of a chain is one 32-byte entry {r, g, b, f} at [generation * capa + chain], written by
wf_shade or by the fused tail and read back by wf_fold or by the tail's own fold; a chunk whose
fused tail starts at generation 1..5 keeps the levels as a word in each of four arrays over the
same bytes instead (levels_packed, device_layout.hpp).  Both forms run here: the words under a tail
from generations 1..5 (the default of these small frames is 4), the packed entries under a tail from
6 or 7 and wherever no tail runs (depth 0 and 1, directional lights, 10 k objects).  The cases are the
smallest frames at which that addressing can go wrong: a frame of whole 8x8 tiles and one of partial
tiles (capa differs from the pixel count), levels written by both writers (the fused tail forced to
start at generations 1..4, so deep levels are sparse), the Fresnel factor taken from the entry, no
level and one level, the passes of RT_ALGO_WAVEFRONT_AA, a skybox scene, a progressive render
resolved after two sample ranges, and a scene of 10 k objects.

Every case is compared with the oracle as test_gpu_parity.py does: BGR bytes equal, f32 within 1e-5
relative of the oracle's f64 colour, rays and shadow rays equal.  The oracle's renders are computed
once per (scene, options) and left unchanged.
"""
import contextlib
import os

import numpy as np
import pytest

import libraytrace as lr
from libraytrace import scenes
from oracle import ref64

pytestmark = pytest.mark.gpu

RTOL = 1e-5
F32_SUBNORMAL_HALF_STEP = 2.0 ** -150          # as test_gpu_path.py: half a step of f32's subnormal grid
WF, AA = lr.RT_ALGO_WAVEFRONT, lr.RT_ALGO_WAVEFRONT_AA

_refs = {}


def oracle(key, spec, **kw):
    k = (key, spec.width, spec.height, spec.max_depth, spec.antialias, tuple(sorted(kw.items())))
    if k not in _refs:
        _refs[k] = ref64.render(spec, **kw)
    return _refs[k]


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


def assert_f32(rgb, r64):
    g = rgb.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        r32 = r64.astype(np.float32).astype(np.float64)
        ok = ((np.isnan(r64) & np.isnan(g)) | (np.isinf(r32) & (r32 == g)) |
              (np.abs(g - r64) <= RTOL * np.abs(r64) + F32_SUBNORMAL_HALF_STEP))
    assert ok.all(), f"{(~ok).sum()} colour components beyond rtol {RTOL}"


def check(rgb, bgr, rays, shadow_rays, ref):
    assert np.array_equal(bgr, ref["bgr"]), f"{(bgr != ref['bgr']).sum()} BGR bytes differ"
    assert_f32(rgb, ref["rgb64"])
    assert (rays, shadow_rays) == (ref["counts"]["rays"], ref["counts"]["shadow_rays"])


def render(ctx, spec, algo=WF, **kw):
    ctx.upload(lr.Scene.deserialize(spec.to_text()))
    o = lr.render_opts(spec.width, spec.height, max_depth=spec.max_depth, spp=spec.antialias, algo=algo, **kw)
    return ctx.render(o)


def check_render(ctx, spec, ref, algo=WF, **kw):
    rgb, bgr, st = render(ctx, spec, algo, **kw)
    check(rgb, bgr, st.rays, st.shadow_rays, ref)
    return rgb, bgr, st


def c3(width, height, depth=8):
    spec = scenes.config3(width, height)
    spec.max_depth = depth
    return spec


# 64x48: whole 8x8 tiles; 61x45: partial tiles, so the chains' stride capa is not the pixel count
@pytest.mark.parametrize("size", [(64, 48), (61, 45)], ids=["64x48", "61x45"])
def test_config3_default_schedule_and_forced_tails(gpu_ctx, size):
    """The default schedule, then the fused tail from generations 1..4 (levels as words), 5, and 6
    and 7 (packed entries): the levels below T are wf_shade's, the sparse ones from T on the
    tail's, and both folds read them."""
    spec = c3(*size)
    ref = oracle("c3", spec)
    check_render(gpu_ctx, spec, ref)
    for T in (1, 2, 3, 4, 5, 6, 7):
        with tuning(gpu_ctx, tail_fuse=T):
            check_render(gpu_ctx, spec, ref)
            gpu_ctx.kernel_times()
            gpu_ctx.render(lr.render_opts(spec.width, spec.height, max_depth=8, spp=1, algo=WF,
                                          flags=lr.RT_OUT_BGR_U8 | lr.RT_TIME_KERNELS))
            kt = gpu_ctx.kernel_times()
        assert kt["tail"][1] == 1 and kt["shade"][1] == T - 1 and kt["fold"][1] == 1, (T, kt)


def test_fresnel_factor_comes_from_the_entry(gpu_ctx):
    spec = scenes.config2_fresnel(80, 45)
    check_render(gpu_ctx, spec, oracle("c2f", spec))


@pytest.mark.parametrize("depth", [0, 1])
def test_no_level_and_one_level(gpu_ctx, depth):
    spec = c3(64, 48, depth)
    check_render(gpu_ctx, spec, oracle("c3", spec))


def test_aa_passes_three_random_samples(gpu_ctx):
    spec = scenes.config3(48, 32)
    spec.antialias = 3
    ref = oracle("c3aa", spec, jitter=1, seed=7, rng=1)
    check_render(gpu_ctx, spec, ref, algo=AA, jitter=lr.RT_JITTER_RANDOM, seed=7)


def test_skybox_chain_scene(gpu_ctx, tmp_path):
    paths = [str(tmp_path / f"f{k}.ppm") for k in range(6)]
    for p, f in zip(paths, scenes.skybox_faces(size=24, seed=4)):
        scenes.write_ppm(p, f)
    spec = scenes.skybox_chain_scene(paths, 48, 32)
    check_render(gpu_ctx, spec, oracle("sky", spec))


def test_progressive_two_ranges_resolved(gpu_ctx):
    spec = scenes.config3(48, 32)
    spec.antialias = 3
    ref = oracle("c3aa", spec, jitter=1, seed=7, rng=1)
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    acc = gpu_ctx.accumulator(lr.render_opts(48, 32, max_depth=spec.max_depth, spp=1, algo=lr.RT_ALGO_AUTO,
                                             jitter=lr.RT_JITTER_RANDOM, seed=7))
    rays = shadow = 0
    for n in (1, 2):
        acc.add(n, AA)
        st = gpu_ctx.stats()
        rays, shadow = rays + st.rays, shadow + st.shadow_rays
    rgb, bgr = acc.resolve()
    acc.close()
    check(rgb, bgr, rays, shadow, ref)


def test_ten_thousand_objects(gpu_ctx):
    spec = scenes.config4(96, 80)
    check_render(gpu_ctx, spec, oracle("c4", spec, threads=min(16, os.cpu_count() or 1)))
