"""RT_ALGO_WAVEFRONT_AA: the wavefront schedule run once per jittered AA sample.

Every sample of a pixel gets its own jitter (ka = key_child(key_pixel(seed, x, y), a),
jx = key_f64(ka, 0), jy = key_f64(ka, 1)) and its own ray tree on the chain schedule;
the samples are summed in f64 in sample order (acc = 0.0; acc = acc + s_a), divided by
spp, rounded once to f32 and quantised from the f64 value.  That is what the oracle
renders with jitter=1, rng=1, so every case is compared with it on five points
(check): BGR bytes equal, f32 within 1e-5 relative (with the subnormal term of
test_gpu_path.py), NaN mask equal, rays and shadow_rays equal, and the library's
verbose line `rtamd: aa passes S, chunks N x R rows, ...` showing that the passes ran.

The oracle's renders are computed once per (scene, spp, seed) and left unchanged.
"""
import contextlib
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import libraytrace as lr
from libraytrace import scenes
from oracle import ref64
import adversarial_scenes

pytestmark = pytest.mark.gpu

RTOL = 1e-5
F32_SUBNORMAL_HALF_STEP = 2.0 ** -150          # as test_gpu_path.py: half a step of f32's subnormal grid
AA = lr.RT_ALGO_WAVEFRONT_AA
AA_LINE = re.compile(r"rtamd: aa passes (\d+), chunks (\d+) x (\d+) rows")
PATH_LINE = re.compile(r"rtamd: path G \d+ T \d+ staged \d+ npix \d+")
GROWN = re.compile(r"rtamd: lane working set grown to (\d+) KB")
RELEASED = re.compile(r"rtamd: lane working set released")

_refs = {}


def oracle(key, spec, spp, seed, **tile):
    """ref64.render(spec with antialias spp, jitter=1, seed, rng=1), once per key."""
    k = (key, spp, seed, tuple(sorted(tile.items())))
    if k not in _refs:
        spec.antialias = spp
        _refs[k] = ref64.render(spec, jitter=1, seed=seed, rng=1, **tile)
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


def opts(spec, spp, seed, algo=AA, jitter=lr.RT_JITTER_RANDOM, **kw):
    return lr.render_opts(spec.width, spec.height, max_depth=spec.max_depth, spp=spp, algo=algo, jitter=jitter,
                          seed=seed, **kw)


def render(ctx, capfd, spec, spp, seed, tune=None, upload=True, **kw):
    """Upload (under the tuning: light_grids acts there) and render under tuning verbose.
    -> (rgb, bgr, st, stderr text of the render)"""
    with tuning(ctx, verbose=1, **(tune or {})):
        if upload:
            ctx.upload(lr.Scene.deserialize(spec.to_text()))
        capfd.readouterr()
        out = ctx.render(opts(spec, spp, seed, **kw))
        err = capfd.readouterr().err
    return out + (err,)


def assert_f32(rgb, r64):
    g = rgb.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        r32 = r64.astype(np.float32).astype(np.float64)
        ok = ((np.isnan(r64) & np.isnan(g)) | (np.isinf(r32) & (r32 == g)) |
              (np.abs(g - r64) <= RTOL * np.abs(r64) + F32_SUBNORMAL_HALF_STEP))
    assert ok.all(), f"{(~ok).sum()} colour components beyond rtol {RTOL}"
    assert np.array_equal(np.isnan(g), np.isnan(r64)), "NaN pixels differ"


def assert_passes(err, spp, chunks=None):
    lines = AA_LINE.findall(err)
    assert len(lines) == 1, err
    assert int(lines[0][0]) == spp, lines
    if chunks is not None:
        assert int(lines[0][1]) == chunks, lines
    assert not PATH_LINE.search(err), err


def check(out, ref, spp, pixels=None, chunks=None):
    """The five points."""
    rgb, bgr, st, err = out
    w3 = ref["bgr"].shape[1]
    assert np.array_equal(bgr[:, :w3], ref["bgr"]), f"{(bgr[:, :w3] != ref['bgr']).sum()} BGR bytes differ"
    assert_f32(rgb, ref["rgb64"])
    assert (st.rays, st.shadow_rays) == (ref["counts"]["rays"], ref["counts"]["shadow_rays"]), \
        (st.rays, st.shadow_rays, ref["counts"])
    assert st.traced_rays == st.rays
    if pixels is not None:
        assert st.pixels == pixels
    assert_passes(err, spp, chunks)
    if chunks is not None:
        assert st.chunks == chunks


def same_bits(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1], b[1])
    assert (a[2].rays, a[2].shadow_rays) == (b[2].rays, b[2].shadow_rays)


# ---- basic parity ----

@pytest.mark.parametrize("spp", [2, 5])
def test_config3_matches_oracle(gpu_ctx, capfd, spp):
    spec = scenes.config3(96, 64, n=300)
    check(render(gpu_ctx, capfd, spec, spp, 7), oracle("c3_96", spec, spp, 7), spp, pixels=96 * 64, chunks=1)


def test_fresnel_directional_planes_match_oracle(gpu_ctx, capfd):
    spec = scenes.config2_fresnel(80, 45)
    check(render(gpu_ctx, capfd, spec, 4, 11), oracle("c2f", spec, 4, 11), 4)


# ---- trees beyond LDS ----

def test_config4_tree_beyond_lds(gpu_ctx, capfd):
    spec = scenes.config4(64, 48)
    out = render(gpu_ctx, capfd, spec, 2, 5)
    m = re.search(r"rtamd: wavefront src (\d+) occ (\d+)", out[3])
    assert m and int(m.group(1)) in (5, 6, 8) and int(m.group(2)) == 11, out[3]      # an LDS-prefix source
    check(out, oracle("c4", spec, 2, 5), 2)


# ---- adversarial scenes ----

@pytest.mark.parametrize("name", ["nan_plane_scene", "coincident_scene", "axis_tie_scene", "extreme_magnitudes_scene"])
def test_adversarial_scenes(gpu_ctx, capfd, name):
    spec = getattr(adversarial_scenes, name)()
    check(render(gpu_ctx, capfd, spec, 3, 23), oracle(name, spec, 3, 23), 3)


def test_negative_zero_and_nan_samples(gpu_ctx, capfd):
    """Samples of -0.0 (background and ambient components): the sum starts with 0.0 + s_0, so
    the pixel is +0.0.  Then a plane with a zero normal, whose hit distance is 0 / 0 for every
    ray: every sample is NaN and so is every pixel."""
    spec = adversarial_scenes.tiny(width=24, height=16)
    spec.background = (-0.0, 0.0, -0.0)
    spec.sphere((0.0, 0.0, -4.0), 1.0, scenes.phong((0.0,) * 3, (0.0,) * 3, 1.0, (0.5, 0.25, -0.0)))
    ref = oracle("neg_zero", spec, 3, 29)
    assert (ref["rgb64"] == 0.0).any() and not np.signbit(ref["rgb64"]).any()
    out = render(gpu_ctx, capfd, spec, 3, 29)
    check(out, ref, 3)
    assert np.array_equal(out[0].view(np.uint32), ref["rgb32"].view(np.uint32)) and not np.signbit(out[0]).any()
    spec.plane((0, 0, 0), (0, 0, 0), scenes.phong((0.1, 0.2, 0.3), (0.2, 0.2, 0.2), 4.0, (0, 0, 1)))
    spec.point_light((3, 3, 3), (1, 1, 1))
    ref = oracle("nan_plane_all", spec, 3, 29)
    assert np.isnan(ref["rgb64"]).all()
    out = render(gpu_ctx, capfd, spec, 3, 29)
    check(out, ref, 3)
    assert np.isnan(out[0]).all()


# ---- sample order ----

def cancelling_spheres():
    """test_gpu_path.py's _cancelling_spheres: unlit Phong spheres whose ambient colours are
    +2^100 and -2^100 in turn over a background of order 1.  A pixel whose samples see both
    signs keeps the background's share only if its samples are added in sample order:
    (2^100 + -2^100) + c is c, (c + -2^100) + 2^100 is 0.  No lights: a chain scene."""
    spec = scenes.SceneSpec(width=48, height=32, antialias=1, max_depth=2, camera=dict(scenes.DEFAULT_CAMERA),
                            background=(0.25, 0.5, 0.75))
    big = 2.0 ** 100
    n = 24
    for i in range(n):
        for j in range(n):
            a = big if (i + j) % 2 == 0 else -big
            spec.sphere((0.4 * (i - 0.5 * n), -0.2 + 0.4 * (j - 0.5 * n), -6.0), 0.18,
                        scenes.phong((0.0,) * 3, (0.0,) * 3, 1.0, (a, 0.5 * a, 0.25 * a)))
    return spec


@pytest.mark.parametrize("compose", [0, 1])
@pytest.mark.parametrize("spp", [3, 5, 16])
def test_sum_is_in_sample_order(gpu_ctx, capfd, spp, compose):
    spec = cancelling_spheres()
    ref = oracle("cancel", spec, spp, 19)
    r64 = ref["rgb64"]
    mixed = (np.abs(r64) < 2.0 ** 90).all(axis=2) & (r64 != np.array(spec.background)).any(axis=2)
    assert mixed.sum() >= 15, mixed.sum()             # pixels where +-2^100 samples cancelled: the order-sensitive ones
    out = render(gpu_ctx, capfd, spec, spp, 19, tune=dict(compose=compose))
    check(out, ref, spp)
    assert np.array_equal(out[0].view(np.uint32), ref["rgb32"].view(np.uint32))     # any other order: another f32 image


# ---- device against device ----

@pytest.mark.parametrize("scene", ["config3", "cancelling"])
def test_same_image_as_the_path_kernel(gpu_ctx, capfd, scene):
    spec, spp, seed = (scenes.config3(96, 64, n=300), 5, 7) if scene == "config3" else (cancelling_spheres(), 5, 19)
    a = render(gpu_ctx, capfd, spec, spp, seed)
    assert_passes(a[3], spp)
    b = render(gpu_ctx, capfd, spec, spp, seed, algo=lr.RT_ALGO_PATH)
    assert PATH_LINE.search(b[3]) and not AA_LINE.search(b[3])
    same_bits(a, b)


# ---- schedule variants ----

THREE_CHUNKS = 128 * 32
VARIANTS = [
    ("three_chunks", dict(chunk_pixels=THREE_CHUNKS), 3),
    ("three_chunks_two_lanes", dict(chunk_pixels=THREE_CHUNKS, lanes=2), 3),
    ("compose", dict(compose=1), 1),
    ("compose_three_chunks_two_lanes", dict(compose=1, chunk_pixels=THREE_CHUNKS, lanes=2), 3),
    ("no_tail", dict(tail_fuse=0), 1),
    ("tail_from_2", dict(tail_fuse=2), 1),
    ("tail_from_2_compose", dict(tail_fuse=2, compose=1), 1),
    ("cam_per_ray", dict(cam=0), 1),
    ("cam_view_grid", dict(cam=3), 1),
    ("no_light_grids", dict(light_grids=0), 1),
    ("event_joins", dict(dev_join=0), 1),
    ("one_stream", dict(split=0), 1),
    ("one_stream_compose_no_tail", dict(split=0, compose=1, tail_fuse=0, chunk_pixels=THREE_CHUNKS), 3),
]


def test_schedule_variants_are_bit_equal(gpu_ctx, capfd):
    """config3 128x96 at depth 8, spp 3: every variant is the oracle's image and, bit for bit,
    the default schedule's."""
    spec = scenes.config3(128, 96)
    assert spec.max_depth == 8
    ref = oracle("c3_128", spec, 3, 31)
    base = render(gpu_ctx, capfd, spec, 3, 31)
    check(base, ref, 3, chunks=1)
    assert re.search(r"cam 3 ", base[3]), base[3]                     # the default takes the view grid
    for name, tune, chunks in VARIANTS:
        out = render(gpu_ctx, capfd, spec, 3, 31, tune=tune)
        try:
            check(out, ref, 3, chunks=chunks)
            same_bits(out, base)
        except AssertionError as e:
            raise AssertionError(f"variant {name}: {e}") from e
        if "cam" in tune:
            assert re.search(r"cam %d " % tune["cam"], out[3]), (name, out[3])
        if "lanes" in tune:
            assert re.search(r"lanes %d," % tune["lanes"], out[3]), (name, out[3])


# ---- geometry of the output ----

def test_tile_offsets_bands_and_pitch(gpu_ctx, capfd):
    spec = scenes.config3(96, 64, n=300)
    full = oracle("c3_96", spec, 3, 7)
    # a tile at an offset, its padded rows ending in a partial dword (dword stores) / at an odd pitch (byte stores)
    for pitch in (3 * 17 + 5, 3 * 17 + 2):
        tile = dict(x0=5, tile_w=17, y0=3, tile_h=13)
        out = render(gpu_ctx, capfd, spec, 3, 7, bgr_pitch=pitch, **tile)
        check(out, oracle("c3_96", spec, 3, 7, **tile), 3, pixels=17 * 13)
        assert np.array_equal(out[1][:, :51], full["bgr"][3:16, 15:66])
        assert (out[1][:, 51:] == 0).all()                 # rt_render writes the row padding as zero (main.rs:42)
    # a padded pitch on the whole frame
    out = render(gpu_ctx, capfd, spec, 3, 7, bgr_pitch=3 * 96 + 8)
    check(out, full, 3)
    assert (out[1][:, 288:] == 0).all()
    # row bands: the rows of the full frame
    out = render(gpu_ctx, capfd, spec, 3, 7, tile_h=20, band=4, band_stride=3, band_phase=1)
    rows = [r for r in range(64) if (r // 4) % 3 == 1][:20]
    assert len(rows) == 20
    assert_passes(out[3], 3)
    assert np.array_equal(out[1], full["bgr"][rows])
    assert np.array_equal(out[0].view(np.uint32), full["rgb32"][rows].view(np.uint32))
    # one output only
    with tuning(gpu_ctx, verbose=0):
        rgb, none, _ = gpu_ctx.render(opts(spec, 3, 7, flags=lr.RT_OUT_RGB_F32), bgr=False)
        assert none is None and np.array_equal(rgb.view(np.uint32), full["rgb32"].view(np.uint32))
        none, bgr, _ = gpu_ctx.render(opts(spec, 3, 7, flags=lr.RT_OUT_BGR_U8), rgb=False)
        assert none is None and np.array_equal(bgr, full["bgr"])


def test_frame_rows_into_a_whole_frame(gpu_ctx, capfd):
    """RT_OUT_FRAME_ROWS: two ranks' row bands straight into one host frame (three chunks each)."""
    spec = scenes.config3(96, 64, n=300)
    full = oracle("c3_96", spec, 3, 7)
    pitch = 3 * 96 + 4
    frame_rgb = np.full((64, 96, 3), np.nan, np.float32)
    frame_bgr = np.full((64, pitch), 0xCD, np.uint8)
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    rays = 0
    with tuning(gpu_ctx, verbose=1, chunk_pixels=96 * 16):
        for r in range(2):
            o = opts(spec, 3, 7, tile_h=32, band=8, band_stride=2, band_phase=r, bgr_pitch=pitch,
                     flags=lr.RT_OUT_RGB_F32 | lr.RT_OUT_BGR_U8 | lr.RT_OUT_FRAME_ROWS)
            capfd.readouterr()
            _, _, st = gpu_ctx.render(o, out=(frame_rgb, frame_bgr))
            assert_passes(capfd.readouterr().err, 3, chunks=2)
            rays += st.rays
    assert np.array_equal(frame_bgr[:, :288], full["bgr"])
    assert np.array_equal(frame_rgb.view(np.uint32), full["rgb32"].view(np.uint32))
    assert rays == full["counts"]["rays"]


def _hip():
    """The HIP runtime librtamd.so is linked against, for device buffers of the test's own: the
    library's handle resolves hipMalloc through its own dependencies (torch bundles another copy,
    which another test of the session may have loaded beside it)."""
    return lr.lib


def test_render_device_leaves_the_padding(gpu_ctx, capfd):
    """rt_render_device into the caller's device buffers: the pixels the oracle's, the row
    padding and the bytes around the rows untouched; statistics read after the call."""
    spec = scenes.config3(96, 64, n=300)
    tile = dict(x0=8, tile_w=40, y0=5, tile_h=30)
    ref = oracle("c3_96", spec, 3, 7, **tile)
    pitch, guard = 3 * 40 + 4, 256
    hip = _hip()
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    n_bgr, n_rgb = guard + 30 * pitch + guard, 30 * 40 * 3 * 4
    h_bgr = np.full(n_bgr, 0xCD, np.uint8)
    h_rgb = np.full(30 * 40 * 3, np.nan, np.float32)
    d_bgr, d_rgb = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d_bgr), n_bgr) == 0 and hip.hipMalloc(ctypes.byref(d_rgb), n_rgb) == 0
    try:
        assert hip.hipMemcpy(d_bgr, h_bgr.ctypes.data, n_bgr, 1) == 0 and hip.hipMemcpy(d_rgb, h_rgb.ctypes.data, n_rgb, 1) == 0
        with tuning(gpu_ctx, verbose=1):
            gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
            capfd.readouterr()
            gpu_ctx.render_device(opts(spec, 3, 7, bgr_pitch=pitch, **tile), d_rgb.value, d_bgr.value + guard)
            st = gpu_ctx.stats()                          # synchronises with the render
            assert_passes(capfd.readouterr().err, 3)
        assert hip.hipMemcpy(h_bgr.ctypes.data, d_bgr, n_bgr, 2) == 0 and hip.hipMemcpy(h_rgb.ctypes.data, d_rgb, n_rgb, 2) == 0
    finally:
        hip.hipFree(d_bgr)
        hip.hipFree(d_rgb)
    rows = h_bgr[guard:guard + 30 * pitch].reshape(30, pitch)
    assert np.array_equal(rows[:, :120], ref["bgr"])
    assert (rows[:, 120:] == 0xCD).all(), "row padding written"
    assert (h_bgr[:guard] == 0xCD).all() and (h_bgr[guard + 30 * pitch:] == 0xCD).all(), "guard bytes written"
    assert_f32(h_rgb.reshape(30, 40, 3), ref["rgb64"])
    assert (st.rays, st.shadow_rays, st.pixels) == (ref["counts"]["rays"], ref["counts"]["shadow_rays"], 40 * 30)


# ---- API ----

@pytest.mark.parametrize("jitter,spp", [(lr.RT_JITTER_RANDOM, 1), (lr.RT_JITTER_CENTER, 4)])
def test_one_sample_or_centre_jitter_is_the_wavefront_render(gpu_ctx, capfd, jitter, spp):
    spec = scenes.config3(96, 64, n=300)
    a = render(gpu_ctx, capfd, spec, spp, 7, jitter=jitter)
    assert not AA_LINE.search(a[3]), a[3]
    b = render(gpu_ctx, capfd, spec, spp, 7, jitter=jitter, algo=lr.RT_ALGO_WAVEFRONT)
    same_bits(a, b)
    assert a[2].traced_rays == b[2].traced_rays == a[2].rays // spp
    spec.antialias = spp
    ref = ref64.render(spec, jitter=jitter, seed=7, rng=1)
    assert np.array_equal(a[1], ref["bgr"]) and a[2].rays == ref["counts"]["rays"]


def test_refusals(gpu_ctx):
    gpu_ctx.upload(lr.Scene.deserialize(scenes.stochastic(32, 32).to_text()))
    with pytest.raises(lr.RtError) as e:
        gpu_ctx.render(lr.render_opts(32, 32, spp=2, algo=AA, jitter=lr.RT_JITTER_RANDOM))
    assert e.value.code == lr.RT_E_UNSUPPORTED and "RT_ALGO_PATH" in str(e.value)
    spec = scenes.config2(32, 32)
    for k in range(33 - len(spec.lights)):
        spec.point_light((0.1 * k, 4.0, 1.0), (0.01, 0.01, 0.01))
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    with pytest.raises(lr.RtError) as e:
        gpu_ctx.render(lr.render_opts(32, 32, spp=2, algo=AA, jitter=lr.RT_JITTER_RANDOM))
    assert e.value.code == lr.RT_E_UNSUPPORTED and "32 lights" in str(e.value)
    # the other chain schedules answer as before
    gpu_ctx.upload(lr.Scene.deserialize(scenes.config2(32, 32).to_text()))
    with pytest.raises(lr.RtError) as e:
        gpu_ctx.render(lr.render_opts(32, 32, spp=2, algo=lr.RT_ALGO_WAVEFRONT, jitter=lr.RT_JITTER_RANDOM))
    assert e.value.code == lr.RT_E_UNSUPPORTED


def test_auto_takes_the_passes_only_under_aa_wavefront(gpu_ctx, capfd):
    assert "aa_wavefront" == lr.tuning_keys()[-1] and gpu_ctx.get_tuning("aa_wavefront") == 0
    spec = scenes.config3(96, 64, n=300)
    ref = oracle("c3_96", spec, 3, 7)
    on = render(gpu_ctx, capfd, spec, 3, 7, tune=dict(aa_wavefront=1), algo=lr.RT_ALGO_AUTO)
    check(on, ref, 3)
    off = render(gpu_ctx, capfd, spec, 3, 7, tune=dict(aa_wavefront=0), algo=lr.RT_ALGO_AUTO)
    assert PATH_LINE.search(off[3]) and not AA_LINE.search(off[3]), off[3]
    same_bits(on, off)


def test_reserved_render_allocates_nothing(capfd):
    """rt_ctx_reserve with the render's options sizes the working set with its running sums:
    the render after it neither grows nor releases a working set (the library's verbose lines)."""
    spec = scenes.config3(96, 64, n=300)
    ref = oracle("c3_96", spec, 3, 7)
    with lr.Context(0, tuning={"verbose": 1}) as ctx:
        ctx.upload(lr.Scene.deserialize(spec.to_text()))
        # a centre-jitter render first: its working set has no running sums, the reserve must grow it
        ctx.render(opts(spec, 1, 7, jitter=lr.RT_JITTER_CENTER))
        capfd.readouterr()
        ctx.reserve(opts(spec, 3, 7), host=True)
        err = capfd.readouterr().err
        assert len(GROWN.findall(err)) == 1 and len(RELEASED.findall(err)) == 1, err
        rgb, bgr, st = ctx.render(opts(spec, 3, 7))
        err = capfd.readouterr().err
        assert not GROWN.search(err) and not RELEASED.search(err), err
        check((rgb, bgr, st, err), ref, 3)


def test_statistics_read_late(capfd):
    """rt_ctx_stats after a render without an rt_stats, after a reserve that replaces the working
    set and after an upload of another scene: still the oracle's totals over all passes."""
    spec = scenes.config3(96, 64, n=300)
    ref = oracle("c3_96", spec, 3, 7)
    with lr.Context(0, tuning={"verbose": 1}) as ctx:
        ctx.upload(lr.Scene.deserialize(spec.to_text()))
        capfd.readouterr()
        rgb, bgr, st = ctx.render(opts(spec, 3, 7), stats=False)
        assert st is None
        assert_passes(capfd.readouterr().err, 3, chunks=1)
        ctx.reserve(lr.render_opts(512, 384, max_depth=8, spp=3, algo=AA, jitter=lr.RT_JITTER_RANDOM))
        assert RELEASED.search(capfd.readouterr().err)
        ctx.upload(lr.Scene.deserialize(scenes.config2(40, 24).to_text()))
        for _ in range(2):
            st = ctx.stats()
            assert (st.rays, st.shadow_rays, st.pixels, st.chunks) == \
                (ref["counts"]["rays"], ref["counts"]["shadow_rays"], 96 * 64, 1)
            assert st.traced_rays == st.rays
        # the queue sizes are the last pass's: one pass's rays at most, a pixel's camera ray not among them
        q, s = ctx.generation_counts()
        assert q[0] == 0 and 0 < sum(q) < ref["counts"]["rays"] - ref["counts"]["shadow_rays"] - 2 * 96 * 64
        assert np.array_equal(bgr, ref["bgr"])


def test_kernel_times_count_a_camera_pass_per_sample_and_chunk(gpu_ctx, capfd):
    spec = scenes.config3(128, 96)
    ref = oracle("c3_128", spec, 3, 31)
    flags = lr.RT_OUT_RGB_F32 | lr.RT_OUT_BGR_U8 | lr.RT_TIME_KERNELS
    for compose in (0, 1):
        gpu_ctx.kernel_times()
        out = render(gpu_ctx, capfd, spec, 3, 31, tune=dict(chunk_pixels=THREE_CHUNKS, compose=compose), flags=flags)
        check(out, ref, 3, chunks=3)
        kt = gpu_ctx.kernel_times()
        assert kt["camera"][1] == 3 * 3
        assert kt["tally"][1] == 3 * 3                    # every pass tallies its own rays
        assert kt["compose"][1] == 3 + 9 * compose        # accum_resolve per chunk (+ the row-ordered sums per pass)


# ---- CLI ----

def test_cli_algo_wavefront_aa(gpu_ctx, tmp_path):
    spec = scenes.config3(80, 48, n=300)
    spec.antialias = 3
    scene = str(tmp_path / "scene.txt")
    with open(scene, "w") as f:
        f.write(spec.to_text())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "rust-raytrace_amd", "raytrace")
    out = str(tmp_path / "cli.bmp")
    r = subprocess.run([exe, "--scene", scene, "--out", out, "--algo", "wavefront-aa", "--jitter", "random", "--spp", "3",
                        "--seed", "77", "--max-depth", str(spec.max_depth)], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stdout + r.stderr
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    hdr, pitch = lr.bmp_header(80, 48)
    _, bgr, st = gpu_ctx.render(opts(spec, 3, 77, bgr_pitch=pitch), rgb=False)
    lib_bmp = str(tmp_path / "lib.bmp")
    lr.write_bmp(lib_bmp, 80, 48, bgr, pitch)
    assert open(out, "rb").read() == open(lib_bmp, "rb").read()
    assert f"{st.rays} rays" in r.stderr, r.stderr
    ref = oracle("c3_80", spec, 3, 77)
    assert np.array_equal(bgr[:, :240], ref["bgr"])
