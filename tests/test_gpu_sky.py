"""SkyboxBackground on the chain schedules.

A skybox scene whose objects, lights and camera are chain classes renders on
RT_ALGO_WAVEFRONT, RT_ALGO_WAVEFRONT_BRUTE, RT_ALGO_WAVEFRONT_AA and both megakernels.  A ray that
misses takes the skybox's colour in its direction (raytrace.rs:234-256): a later generation's as
its chain's terminal, a camera ray's as the pixel (the average of its spp identical centre-jitter
samples, or one jittered sample of the running sum).  Every case is compared with the oracle on
BGR bytes (equal), f32 (1e-5 relative with the subnormal term of test_gpu_path.py), the NaN mask
(equal) and rays / shadow_rays (equal); schedule variants are compared bit for bit with the
default schedule's render as well.

The oracle's renders are computed once per (scene, options) and left unchanged.
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

pytestmark = pytest.mark.gpu

RTOL = 1e-5
F32_SUBNORMAL_HALF_STEP = 2.0 ** -150          # as test_gpu_path.py: half a step of f32's subnormal grid
CENTER, RANDOM = lr.RT_JITTER_CENTER, lr.RT_JITTER_RANDOM
WF, WFB, AA = lr.RT_ALGO_WAVEFRONT, lr.RT_ALGO_WAVEFRONT_BRUTE, lr.RT_ALGO_WAVEFRONT_AA
LDS, GLOBAL, PATH, AUTO = lr.RT_ALGO_BRUTE_LDS, lr.RT_ALGO_BRUTE_GLOBAL, lr.RT_ALGO_PATH, lr.RT_ALGO_AUTO
CHAIN_ALGOS = [WF, WFB, AA, LDS, GLOBAL]
WF_LINE = re.compile(r"rtamd: wavefront src (\d+) occ (\d+) cam (\d+)")
PATH_LINE = re.compile(r"rtamd: path G \d+ T \d+ staged \d+ npix \d+")
GROWN = re.compile(r"rtamd: lane working set grown")

_refs = {}


def write_faces(directory, faces, tag="f"):
    paths = [str(directory / f"{tag}{k}.ppm") for k in range(6)]
    for p, f in zip(paths, faces):
        scenes.write_ppm(p, f)
    return paths


@pytest.fixture(scope="module")
def sky(tmp_path_factory):
    """Six 24x24 faces on disk (seed 4: sky pixels whose three-sample average is not the sample,
    asserted in test_centre_jitter_averages_the_sky_samples)."""
    return write_faces(tmp_path_factory.mktemp("sky"), scenes.skybox_faces(size=24, seed=4))


def oracle(key, spec, spp, jitter, seed=7, **kw):
    k = (key, spp, jitter, seed, tuple(sorted(kw.items())))
    if k not in _refs:
        spec.antialias = spp
        _refs[k] = ref64.render(spec, jitter=jitter, seed=seed, rng=1, **kw)
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


def opts(spec, spp, jitter, seed=7, algo=WF, **kw):
    return lr.render_opts(spec.width, spec.height, max_depth=kw.pop("max_depth", spec.max_depth), spp=spp, algo=algo,
                          jitter=jitter, seed=seed, **kw)


def render(ctx, capfd, spec, spp, jitter, seed=7, algo=WF, tune=None, upload=True, **kw):
    """Upload (under the tuning: light_grids and cam_grid act there) and render under tuning
    verbose -> (rgb, bgr, st, stderr text of the render)."""
    with tuning(ctx, verbose=1, **(tune or {})):
        if upload:
            ctx.upload(lr.Scene.deserialize(spec.to_text()))
        capfd.readouterr()
        out = ctx.render(opts(spec, spp, jitter, seed, algo, **kw))
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


def check(out, ref):
    rgb, bgr, st = out[:3]
    w3 = ref["bgr"].shape[1]
    assert np.array_equal(bgr[:, :w3], ref["bgr"]), f"{(bgr[:, :w3] != ref['bgr']).sum()} BGR bytes differ"
    assert_f32(rgb, ref["rgb64"])
    assert (st.rays, st.shadow_rays) == (ref["counts"]["rays"], ref["counts"]["shadow_rays"]), \
        (st.rays, st.shadow_rays, ref["counts"])


def same_bits(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "f32 bits differ"
    assert np.array_equal(a[1], b[1]), "BGR bytes differ"
    assert (a[2].rays, a[2].shadow_rays) == (b[2].rays, b[2].shadow_rays)


def on_chain_schedule(err):
    assert WF_LINE.search(err) and not PATH_LINE.search(err), err


# ---- 1. every chain algorithm (each raises RT_E_UNSUPPORTED without the feature) ----

@pytest.mark.parametrize("algo", CHAIN_ALGOS)
def test_chain_algorithms_render_the_skybox(gpu_ctx, capfd, sky, algo):
    spec = scenes.skybox_chain_scene(sky, 96, 64)
    ref = oracle("chain", spec, 1, CENTER)
    sky_px = (ref["rgb64"] != oracle("chain_d0", spec, 1, CENTER, max_depth=0)["rgb64"]).any(axis=2)
    assert sky_px.sum() > 100                      # pixels whose mirror images go on past depth 1
    out = render(gpu_ctx, capfd, spec, 1, CENTER, algo=algo)
    check(out, ref)
    assert not PATH_LINE.search(out[3]), out[3]
    assert out[2].traced_rays == out[2].rays


def test_auto_plans_a_skybox_chain_scene_on_the_wavefront(gpu_ctx, capfd, sky):
    spec = scenes.skybox_chain_scene(sky, 96, 64)
    out = render(gpu_ctx, capfd, spec, 1, CENTER, algo=AUTO)
    on_chain_schedule(out[3])
    check(out, oracle("chain", spec, 1, CENTER))
    # the same plan as the same scene with a solid background
    solid = scenes.skybox_chain_scene(sky, 96, 64)
    solid.skybox = None
    solid.background = (0.1, 0.2, 0.3)
    b = render(gpu_ctx, capfd, solid, 1, CENTER, algo=AUTO)
    assert WF_LINE.search(b[3]).groups() == WF_LINE.search(out[3]).groups()
    # Sampling issues no Scene::intersect: the same rays and queue sizes as the solid scene's
    assert (out[2].rays, out[2].shadow_rays, out[2].chunks) == (b[2].rays, b[2].shadow_rays, b[2].chunks)
    q_solid = gpu_ctx.generation_counts()
    render(gpu_ctx, capfd, spec, 1, CENTER, algo=AUTO)
    q_sky = gpu_ctx.generation_counts()
    assert q_sky == q_solid and sum(q_sky[0]) > 0


# ---- 2. the path kernel's bits ----

@pytest.mark.parametrize("algo,jitter,spp", [(WF, CENTER, 1), (WF, CENTER, 3), (LDS, CENTER, 3), (WF, RANDOM, 1),
                                             (AA, RANDOM, 3), (AA, RANDOM, 5)])
def test_same_bits_as_the_path_kernel(gpu_ctx, capfd, sky, algo, jitter, spp):
    spec = scenes.skybox_chain_scene(sky, 96, 64)
    a = render(gpu_ctx, capfd, spec, spp, jitter, algo=algo)
    assert not PATH_LINE.search(a[3]), a[3]
    b = render(gpu_ctx, capfd, spec, spp, jitter, algo=PATH)
    assert PATH_LINE.search(b[3]), b[3]
    same_bits(a, b)
    check(a, oracle("chain", spec, spp, jitter))


# ---- 3. face edges and ties ----

def edge_faces():
    """test_gpu_path.py's _edge_faces: 1x1, 2x2 and non-square 5x3 / 3x5 texels, no texel black."""
    rng = scenes.SplitMix64(9)
    faces = []
    for h, w in [(1, 1), (2, 2), (3, 5), (5, 3), (2, 2), (1, 1)]:
        faces.append(np.array([1 + rng.next() % 255 for _ in range(h * w * 3)], np.uint8).reshape(h, w, 3))
    return faces


def edge_scene(paths):
    """33x16, the camera at the origin looking down -z: columns 8 and 24 look along |dx| == |dz|."""
    spec = scenes.SceneSpec(width=33, height=16, antialias=1, max_depth=4, skybox=paths,
                            camera={"ctor": "new", "position": (0, 0, 0), "look": (0, 0, -1), "up": (0, 1, 0),
                                    "im_dist": 1.0})
    spec.sphere((0.0, 0.0, -6.0), 1.0, scenes.phong((0.1, 0.1, 0.1), (0.8, 0.8, 0.8), 64.0, (0.0, 0.0, 0.0)))
    spec.sphere((0.45, 0.3, -3.0), 0.3, scenes.fresnel((0.1, 0.1, 0.1), (0.9, 0.9, 0.9), 64.0, (0.0, 0.0, 0.0), 1.4))
    spec.point_light((-10.0, 10.0, 5.0), (0.8, 0.8, 0.8))
    return spec


@pytest.mark.parametrize("faces", ["edge", "extremes"])
def test_face_edges_and_ties(gpu_ctx, capfd, tmp_path, faces):
    fs = edge_faces()
    if faces == "extremes":                        # one face of texel values 0 and 255 only (the camera looks at nz)
        fs[5] = np.array([[[0, 255, 0], [255, 0, 255]], [[255, 255, 0], [0, 0, 255]]], np.uint8)
    spec = edge_scene(write_faces(tmp_path, fs, "e"))
    ref = oracle(faces, spec, 1, CENTER, seed=13)
    if faces == "edge":                            # on the oracle first: a wrong tie rule must not hide
        black = (ref["rgb64"] == 0.0).all(axis=2)
        assert black[:, 8].all() and black[:, 24].all() and black.sum() >= spec.height
    # (random jitter with several samples is RT_ALGO_WAVEFRONT_AA's alone among the chain algorithms;
    # RT_ALGO_WAVEFRONT takes one jittered sample, the megakernels centre jitter only)
    for algo, jitter, spp in [(WF, CENTER, 1), (AA, CENTER, 1), (LDS, CENTER, 1), (AA, RANDOM, 3), (WF, RANDOM, 1)]:
        out = render(gpu_ctx, capfd, spec, spp, jitter, seed=13, algo=algo)
        assert not PATH_LINE.search(out[3]), out[3]
        try:
            check(out, oracle(faces, spec, spp, jitter, seed=13))
        except AssertionError as e:
            raise AssertionError(f"algo {algo} jitter {jitter} spp {spp}: {e}") from e


# ---- 4. centre jitter, several samples: (c + c + c) / 3 is not c ----

@pytest.mark.parametrize("spp", [3, 7])
def test_centre_jitter_averages_the_sky_samples(gpu_ctx, capfd, sky, spp):
    spec = scenes.skybox_chain_scene(sky, 96, 64)
    one, ref = oracle("chain", spec, 1, CENTER), oracle("chain", spec, spp, CENTER)
    spec0 = scenes.SceneSpec(width=96, height=64, max_depth=4, camera=dict(spec.camera), skybox=list(sky))
    camera_miss = (oracle("empty", spec0, 1, CENTER)["rgb64"] == one["rgb64"]).all(axis=2)
    assert ((ref["rgb64"] != one["rgb64"]).any(axis=2) & camera_miss).any()   # else the case could not tell
    for algo, tune in [(WF, {}), (WF, dict(compose=1)), (WFB, {}), (LDS, {})]:
        out = render(gpu_ctx, capfd, spec, spp, CENTER, algo=algo, tune=tune)
        check(out, ref)
        assert np.array_equal(out[0].view(np.uint32), ref["rgb32"].view(np.uint32)), (algo, tune)


def test_texel_lerp_order_is_pinned_by_cancellation(gpu_ctx, capfd, sky):
    """The bilinear sample's last f64 bit (lerp over y, then over x) does not reach an f32 pixel by
    itself.  Here it does: a mirror of specular 2^40 and ambient -2^40 c, with c the sky colour its
    centre pixel reflects (read from the oracle's render of the same mirrors with specular 1), is
    exactly 0.0 at that pixel, 2^40 ulp(c) ~ 1e-4 if the sample differs in its last bit."""
    K, n = 2.0 ** 40, 8

    def build(mats):
        spec = scenes.SceneSpec(width=64, height=48, antialias=1, max_depth=0, skybox=list(sky),
                                camera={"ctor": "new", "position": (0, 0, 0), "look": (0, 0, -1), "up": (0, 1, 0),
                                        "im_dist": 1.0})
        for i, m in enumerate(mats):
            spec.sphere((-3.5 + i, 0.6 * (i % 3 - 1), -3.0), 0.45, m)
        return spec

    z3 = (0.0,) * 3
    ids = oracle("lerp_ids", build([scenes.phong(z3, z3, 1.0, (i + 2.0, 0.0, 0.0)) for i in range(n)]), 1, CENTER)
    ones = oracle("lerp_ones", build([scenes.phong(z3, (1.0,) * 3, 1.0, z3)] * n), 1, CENTER)
    px, mats = [], []
    for i in range(n):
        # a pixel of mirror i whose reflection is the sky's colour (depth 0: a neighbour's would be 0)
        ys, xs = np.nonzero((ids["rgb64"][:, :, 0] == i + 2.0) & (ones["rgb64"] > 0.0).all(axis=2))
        assert len(ys) > 10
        y, x = int(ys[len(ys) // 2]), int(xs[len(ys) // 2])
        c = ones["rgb64"][y, x]
        px.append((y, x))
        mats.append(scenes.phong(z3, (K,) * 3, 1.0, tuple(-K * float(v) for v in c)))
    spec = build(mats)
    ref = oracle("lerp_cancel", spec, 1, CENTER)
    assert all((ref["rgb64"][y, x] == 0.0).all() for y, x in px)
    assert (np.abs(ref["rgb64"]) > 1.0).any()                   # ... and 2^40 (c' - c) around them
    for algo, tune in [(WF, {}), (WF, dict(tail_fuse=0, compose=1)), (LDS, {}), (AA, {})]:
        out = render(gpu_ctx, capfd, spec, 1, CENTER, algo=algo, tune=tune)
        check(out, ref)
        assert all((out[0][y, x] == 0.0).all() for y, x in px), (algo, tune, [out[0][y, x] for y, x in px])


# ---- 5. every sink ----

def sink_scene(sky):
    """config3's 1000 spheres and two point lights (every light gridded, the whole tree in LDS: the
    fused tail runs) under the skybox, every fifth sphere a mirror."""
    spec = scenes.config3(128, 96)
    spec.skybox = list(sky)
    for o in spec.objects[::5]:
        o["material"] = scenes.phong((0.05, 0.05, 0.05), (0.9, 0.9, 0.9), 64.0, (0.0, 0.0, 0.0))
    return spec


THREE_CHUNKS = 128 * 32
SINKS = [
    ("compose_0", dict(compose=0)), ("compose_1", dict(compose=1)),
    ("cam_0", dict(cam=0)), ("cam_3", dict(cam=3)), ("cam_0_compose", dict(cam=0, compose=1)),
    ("tail_1", dict(tail_fuse=1)), ("tail_2", dict(tail_fuse=2)), ("tail_0", dict(tail_fuse=0)),
    ("tail_2_compose", dict(tail_fuse=2, compose=1)), ("tail_0_compose", dict(tail_fuse=0, compose=1)),
    ("split_0", dict(split=0)), ("bstreams_1", dict(bstreams=1)),
    ("three_chunks", dict(chunk_pixels=THREE_CHUNKS)), ("three_chunks_compose", dict(chunk_pixels=THREE_CHUNKS, compose=1)),
    ("lanes_2", dict(chunk_pixels=THREE_CHUNKS, lanes=2)),
    ("sparse_0", dict(sparse_out=0)), ("sparse_1", dict(sparse_out=1)),
    ("src_2", dict(src=2)), ("src_8", dict(src=8, src_occ=11)),
]
NOT_FOR_AA = ("sparse_0", "sparse_1")
TIMED = lr.RT_OUT_RGB_F32 | lr.RT_OUT_BGR_U8 | lr.RT_TIME_KERNELS


@pytest.mark.parametrize("algo,jitter,spp", [(WF, CENTER, 1), (AA, RANDOM, 3)])
def test_every_sink_is_bit_equal(gpu_ctx, capfd, sky, algo, jitter, spp):
    spec = sink_scene(sky)
    assert spec.max_depth == 8
    ref = oracle("sink", spec, spp, jitter, seed=31)
    base = render(gpu_ctx, capfd, spec, spp, jitter, seed=31, algo=algo)
    check(base, ref)
    assert WF_LINE.search(base[3]).group(1) == "9", base[3]           # the whole tree in LDS
    for name, tune in SINKS:
        if algo == AA and name in NOT_FOR_AA:
            continue
        gpu_ctx.kernel_times()
        out = render(gpu_ctx, capfd, spec, spp, jitter, seed=31, algo=algo, tune=tune, flags=TIMED)
        kt = gpu_ctx.kernel_times()
        try:
            check(out, ref)
            same_bits(out, base)
            if "tail_fuse" in tune:                                   # the tail really ran (or did not)
                assert (kt["tail"][1] > 0) == (tune["tail_fuse"] > 0), kt
            if "cam" in tune:
                assert WF_LINE.search(out[3]).group(3) == str(tune["cam"]), out[3]
            if "src" in tune:
                assert WF_LINE.search(out[3]).group(1) == str(tune["src"]), out[3]
            if "chunk_pixels" in tune:
                assert out[2].chunks == 3
        except AssertionError as e:
            raise AssertionError(f"variant {name}: {e}") from e
    if algo == WF:
        out = render(gpu_ctx, capfd, spec, spp, jitter, seed=31, algo=WFB)
        check(out, ref)
        same_bits(out, base)


# ---- 6. depths: chains that end by the cut-off and chains that end on the sky ----

def facing_mirrors(sky):
    """Two perfect mirror spheres of radius 5 almost touching, seen from in front of the gap: a ray
    that enters the gap bounces between them (rays of depth 10 still hit) until it leaves for the sky."""
    spec = scenes.SceneSpec(width=64, height=48, antialias=1, max_depth=8, skybox=list(sky),
                            camera={"ctor": "new", "position": (0.0, 0.0, 5.0), "look": (0.0, 0.0, -1.0),
                                    "up": (0.0, 1.0, 0.0), "im_dist": 1.5})
    mirror = scenes.phong((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 64.0, (0.02, 0.03, 0.04))
    spec.sphere((-5.02, 0.0, 0.0), 5.0, mirror)
    spec.sphere((5.02, 0.0, 0.0), 5.0, mirror)
    spec.point_light((0.0, 10.0, 5.0), (0.8, 0.8, 0.8))
    return spec


def test_depths(gpu_ctx, capfd, sky):
    spec = facing_mirrors(sky)
    npix = spec.width * spec.height
    # the oracle's nearest queries at max_depth D are the rays of depths 0 .. D + 1, so Q[k], the
    # rays of depth k, is the difference of two renders' counts
    near = []
    for d in range(10):
        c = oracle("mirrors", spec, 1, CENTER, max_depth=d)["counts"]
        near.append(c["rays"] - c["shadow_rays"])
    Q = [npix, near[0] - npix] + [near[d] - near[d - 1] for d in range(1, 10)]
    # every surface is a perfect mirror (ks = 1: no chain ends insignificant), so a ray of depth
    # k <= max_depth that spawns none missed: chains end on the sky at depths 1, 2 and beyond ...
    assert Q[1] > Q[2] > Q[3] > 0, Q
    # ... and depth-9 rays still hit (they spawn depth-10 rays): at max_depth 8 those end by the cut-off
    assert Q[10] > 0 and Q[2] > 0, Q
    for d in (0, 1, 8):
        ref = oracle("mirrors", spec, 1, CENTER, max_depth=d)
        for algo, tune in [(WF, {}), (WF, dict(tail_fuse=0)), (WF, dict(compose=1)), (LDS, {}), (AA, {})]:
            try:
                check(render(gpu_ctx, capfd, spec, 1, CENTER, algo=algo, tune=tune, max_depth=d), ref)
            except AssertionError as e:
                raise AssertionError(f"max_depth {d} algo {algo} {tune}: {e}") from e


# ---- 7. geometry: the camera ray of a sky pixel comes from the frame's coordinates ----

def _device_buffers(n_bgr, n_rgb):
    hip = lr.lib
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    d_bgr, d_rgb = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d_bgr), n_bgr) == 0 and hip.hipMalloc(ctypes.byref(d_rgb), n_rgb) == 0
    return hip, d_bgr, d_rgb


@pytest.mark.parametrize("algo,jitter,spp", [(WF, CENTER, 1), (AA, RANDOM, 3)])
@pytest.mark.parametrize("compose", [0, 1])
def test_geometry(gpu_ctx, capfd, sky, algo, jitter, spp, compose):
    spec = scenes.skybox_chain_scene(sky, 64, 48)
    spec.camera = dict(spec.camera, look=(0.0, 0.1, -1.0))         # sky in the tile and in the bands:
    empty = scenes.SceneSpec(width=64, height=48, max_depth=4, camera=dict(spec.camera), skybox=list(sky))
    miss = (oracle("chain64", spec, 1, CENTER)["rgb64"] == oracle("empty64", empty, 1, CENTER)["rgb64"]).all(axis=2)
    assert miss[8:28, 16:40].sum() > 100 and miss[[r for r in range(48) if (r // 4) % 3 == 1][:16]].sum() > 100
    assert not miss[8:28, 16:40].all()                             # ... beside pixels that are not sky
    tune = dict(compose=compose)
    full = oracle("chain64", spec, spp, jitter)
    base = render(gpu_ctx, capfd, spec, spp, jitter, algo=algo, tune=tune)
    check(base, full)
    f_rgb, f_bgr = base[0].view(np.uint32), base[1]
    # a tile at an offset, padded pitch
    tile = dict(x0=16, tile_w=24, y0=8, tile_h=20)
    out = render(gpu_ctx, capfd, spec, spp, jitter, algo=algo, tune=tune, upload=False, bgr_pitch=3 * 24 + 5, **tile)
    check(out, oracle("chain64", spec, spp, jitter, **tile))
    assert np.array_equal(out[1][:, :72], f_bgr[8:28, 48:120]) and (out[1][:, 72:] == 0).all()
    assert np.array_equal(out[0].view(np.uint32), f_rgb[8:28, 16:40])
    # row bands
    out = render(gpu_ctx, capfd, spec, spp, jitter, algo=algo, tune=tune, upload=False, tile_h=16, band=4, band_stride=3,
                 band_phase=1)
    rows = [r for r in range(48) if (r // 4) % 3 == 1][:16]
    assert len(rows) == 16
    assert np.array_equal(out[1], f_bgr[rows]) and np.array_equal(out[0].view(np.uint32), f_rgb[rows])
    # RT_OUT_FRAME_ROWS: two ranks' bands into one frame
    pitch = 3 * 64 + 4
    frame_rgb = np.full((48, 64, 3), np.nan, np.float32)
    frame_bgr = np.full((48, pitch), 0xCD, np.uint8)
    with tuning(gpu_ctx, chunk_pixels=64 * 8, **tune):
        for r in range(2):
            o = opts(spec, spp, jitter, algo=algo, tile_h=24, band=8, band_stride=2, band_phase=r, bgr_pitch=pitch,
                     flags=lr.RT_OUT_RGB_F32 | lr.RT_OUT_BGR_U8 | lr.RT_OUT_FRAME_ROWS)
            gpu_ctx.render(o, out=(frame_rgb, frame_bgr))
    assert np.array_equal(frame_bgr[:, :192], f_bgr[:, :192]) and np.array_equal(frame_rgb.view(np.uint32), f_rgb)
    # rt_render_device into the caller's padded device buffers
    tile = dict(x0=16, tile_w=24, y0=8, tile_h=20)
    pitch, guard = 3 * 24 + 4, 256
    n_bgr, n_rgb = guard + 20 * pitch + guard, 20 * 24 * 3 * 4
    h_bgr = np.full(n_bgr, 0xCD, np.uint8)
    h_rgb = np.full(20 * 24 * 3, np.nan, np.float32)
    hip, d_bgr, d_rgb = _device_buffers(n_bgr, n_rgb)
    try:
        assert hip.hipMemcpy(d_bgr, h_bgr.ctypes.data, n_bgr, 1) == 0 and hip.hipMemcpy(d_rgb, h_rgb.ctypes.data, n_rgb, 1) == 0
        with tuning(gpu_ctx, **tune):
            gpu_ctx.render_device(opts(spec, spp, jitter, algo=algo, bgr_pitch=pitch, **tile), d_rgb.value, d_bgr.value + guard)
            st = gpu_ctx.stats()                              # synchronises with the render
        assert hip.hipMemcpy(h_bgr.ctypes.data, d_bgr, n_bgr, 2) == 0 and hip.hipMemcpy(h_rgb.ctypes.data, d_rgb, n_rgb, 2) == 0
    finally:
        hip.hipFree(d_bgr)
        hip.hipFree(d_rgb)
    rows = h_bgr[guard:guard + 20 * pitch].reshape(20, pitch)
    assert np.array_equal(rows[:, :72], f_bgr[8:28, 48:120])
    assert (rows[:, 72:] == 0xCD).all(), "row padding written"
    assert (h_bgr[:guard] == 0xCD).all() and (h_bgr[guard + 20 * pitch:] == 0xCD).all(), "guard bytes written"
    assert np.array_equal(h_rgb.view(np.uint32).reshape(20, 24, 3), f_rgb[8:28, 16:40])
    ref = oracle("chain64", spec, spp, jitter, **tile)
    assert (st.rays, st.shadow_rays) == (ref["counts"]["rays"], ref["counts"]["shadow_rays"])


# ---- 8, 9. no lights; no objects ----

@pytest.mark.parametrize("what", ["no_lights", "no_objects"])
def test_degenerate_scenes(gpu_ctx, capfd, sky, what):
    spec = scenes.skybox_chain_scene(sky, 64, 48)
    spec.lights = []
    if what == "no_objects":
        spec.objects = []
    for algo, jitter, spp, tune in [(WF, CENTER, 1, {}), (WF, CENTER, 3, dict(compose=1)), (WFB, CENTER, 1, {}),
                                    (AA, RANDOM, 3, {}), (AA, RANDOM, 3, dict(compose=1)), (LDS, CENTER, 1, {}),
                                    (GLOBAL, CENTER, 3, {})]:
        ref = oracle(what, spec, spp, jitter)
        out = render(gpu_ctx, capfd, spec, spp, jitter, algo=algo, tune=tune)
        try:
            check(out, ref)
        except AssertionError as e:
            raise AssertionError(f"algo {algo} spp {spp} {tune}: {e}") from e
        assert ref["counts"]["shadow_rays"] == 0
        if what == "no_objects":
            assert out[2].rays == 64 * 48 * spp and (ref["rgb64"] > 0.0).any()


# ---- 10. lifecycle ----

@pytest.mark.parametrize("algo,jitter,spp", [(WF, CENTER, 1), (AA, RANDOM, 3)])
def test_reserved_render_allocates_nothing(capfd, sky, algo, jitter, spp):
    spec = scenes.skybox_chain_scene(sky, 96, 64)
    ref = oracle("chain", spec, spp, jitter)
    with lr.Context(0, tuning={"verbose": 1}) as ctx:
        ctx.upload(lr.Scene.deserialize(spec.to_text()))
        ctx.reserve(opts(spec, spp, jitter, algo=algo), host=True)
        capfd.readouterr()
        out = ctx.render(opts(spec, spp, jitter, algo=algo))
        err = capfd.readouterr().err
        assert not GROWN.search(err), err
        check(out, ref)


def test_statistics_read_late_and_scene_changes(capfd, sky):
    spec = scenes.skybox_chain_scene(sky, 96, 64)
    solid = scenes.skybox_chain_scene(sky, 96, 64)
    solid.skybox = None
    solid.background = (0.3, 0.2, 0.1)
    ref, ref_solid = oracle("chain", spec, 1, CENTER), oracle("chain_solid", solid, 1, CENTER)
    tile = dict(x0=0, tile_w=96, y0=0, tile_h=64)
    hip, d_bgr, d_rgb = _device_buffers(64 * 288, 64 * 96 * 12)
    try:
        with lr.Context(0) as ctx:
            ctx.upload(lr.Scene.deserialize(spec.to_text()))
            ctx.render_device(opts(spec, 1, CENTER, bgr_pitch=288, **tile), d_rgb.value, d_bgr.value)
            ctx.upload(lr.Scene.deserialize(solid.to_text()))          # statistics read late: after an upload
            st = ctx.stats()
            assert (st.rays, st.shadow_rays) == (ref["counts"]["rays"], ref["counts"]["shadow_rays"])
            h_bgr = np.zeros((64, 288), np.uint8)
            assert hip.hipMemcpy(h_bgr.ctypes.data, d_bgr, h_bgr.size, 2) == 0
            assert np.array_equal(h_bgr, ref["bgr"])
            # solid after skybox, and back: no stale background constants or sky state
            for compose in (0, 1):
                with tuning(ctx, compose=compose):
                    for algo, jitter, spp in [(WF, CENTER, 1), (AA, RANDOM, 3)]:
                        check(ctx.render(opts(solid, spp, jitter, algo=algo)), oracle("chain_solid", solid, spp, jitter))
                        ctx.upload(lr.Scene.deserialize(spec.to_text()))
                        check(ctx.render(opts(spec, spp, jitter, algo=algo)), oracle("chain", spec, spp, jitter))
                        ctx.upload(lr.Scene.deserialize(solid.to_text()))
                        check(ctx.render(opts(solid, spp, jitter, algo=algo)), oracle("chain_solid", solid, spp, jitter))
            assert ref_solid["counts"]["rays"] == ref["counts"]["rays"]
    finally:
        hip.hipFree(d_bgr)
        hip.hipFree(d_rgb)


# ---- 11. refusals stay ----

@pytest.mark.parametrize("what", ["transparent", "dof"])
def test_path_only_skybox_scenes_are_still_refused(gpu_ctx, capfd, sky, what):
    if what == "transparent":
        spec = scenes.skybox_scene(sky, 48, 32)
    else:
        spec = scenes.skybox_chain_scene(sky, 48, 32)
        spec.depth_of_field(7.0, 0.15, 2)
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    for algo in CHAIN_ALGOS:
        with pytest.raises(lr.RtError) as e:
            gpu_ctx.render(opts(spec, 1, CENTER, algo=algo))
        assert e.value.code == lr.RT_E_UNSUPPORTED and "RT_ALGO_PATH" in str(e.value)
    out = render(gpu_ctx, capfd, spec, 1, CENTER, algo=AUTO)
    assert PATH_LINE.search(out[3]) and not WF_LINE.search(out[3]), out[3]
    check(out, oracle(what, spec, 1, CENTER))


# ---- 12. CLI ----

@pytest.mark.parametrize("algo,extra,spp,jitter", [("wavefront", ["--jitter", "center"], 1, CENTER),
                                                   ("wavefront-aa", ["--jitter", "random"], 3, RANDOM)])
def test_cli(gpu_ctx, tmp_path, sky, algo, extra, spp, jitter):
    spec = scenes.skybox_chain_scene(sky, 80, 48)
    spec.antialias = spp
    scene = str(tmp_path / "scene.txt")
    with open(scene, "w") as f:
        f.write(spec.to_text())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "rust-raytrace_amd", "raytrace")
    out = str(tmp_path / "cli.bmp")
    r = subprocess.run([exe, "--scene", scene, "--out", out, "--algo", algo, "--spp", str(spp), "--seed", "77",
                        "--max-depth", str(spec.max_depth)] + extra, capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stdout + r.stderr
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    hdr, pitch = lr.bmp_header(80, 48)
    lib_algo = WF if algo == "wavefront" else AA
    _, bgr, st = gpu_ctx.render(opts(spec, spp, jitter, seed=77, algo=lib_algo, bgr_pitch=pitch), rgb=False)
    lib_bmp = str(tmp_path / "lib.bmp")
    lr.write_bmp(lib_bmp, 80, 48, bgr, pitch)
    assert open(out, "rb").read() == open(lib_bmp, "rb").read()
    assert np.array_equal(bgr[:, :240], oracle("chain80", spec, spp, jitter, seed=77)["bgr"])
