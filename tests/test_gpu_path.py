"""Parity of the path kernel (RT_ALGO_PATH, csrc/path_kernel.hip) with the oracle.

The path kernel carries the classes the wavefront chain does not: IndirectPhong
and Transparent materials, AreaLight, DepthOfFieldCamera and random AA jitter
with several samples per pixel.  Random draws are keyed on their place in the
recursion (trace_rng.hpp "keyed RNG"); the oracle's REF_RNG_KEYED mode
draws the same numbers, so:
  * scenes whose random draws feed only + - * / sqrt (random jitter, AreaLight,
    Transparent, Phong, Fresnel) must match BIT FOR BIT: BGR bytes equal, f32
    within 1e-5 relative, ray counts equal (assert_exact);
  * IndirectPhong bounce directions and the DoF lens offset go through cos/sin
    (raytrace.rs:104-105, camera.rs:119), where the device's libm and glibc may
    differ in the last ulp, like pow.  How far that can reach is
    derived from the reference alone (tests/trig_scenes.py, test_oracle_trig.py:
    the oracle with every cos / sin / pow result moved by +-1, +-4 and hashed +-1
    ulp): the ray counts and the NaN mask must equal the oracle's, every BGR byte
    that no perturbation moves must equal the oracle's, and any other byte must be
    one of the perturbed oracles' values (assert_trig_exact);
  * the reference's own render, out.bmp (test_scene.txt, 1024 stochastic
    samples), pins the IndirectPhong path statistically (tests/cornell.py).
Every schedule of the kernel is run and named by the kernel's own verbose line
(`rtamd: path G .. T .. staged .. npix ..`): the tree staged in LDS and read
through the caches, one and several trips of the persistent loop, and 1 to 64
lanes per pixel (tuning path_group).
"""
import contextlib
import re

import numpy as np
import pytest

import libraytrace as lr
from libraytrace import scenes
from oracle import ref64
from cornell import check_out_bmp_statistics, cornell_spec
import adversarial_scenes
import trig_scenes

pytestmark = pytest.mark.gpu

RTOL = 1e-5


def render(ctx, spec, *, jitter=lr.RT_JITTER_RANDOM, seed=7, algo=lr.RT_ALGO_AUTO, **kw):
    ctx.upload(lr.Scene.deserialize(spec.to_text()))
    o = lr.render_opts(spec.width, spec.height, max_depth=spec.max_depth, spp=spec.antialias, algo=algo,
                       jitter=jitter, seed=seed)
    for k, v in kw.items():
        setattr(o, k, v)
    return ctx.render(o)


def oracle(spec, *, jitter=1, seed=7, **kw):
    return ref64.render(spec, jitter=jitter, seed=seed, rng=1, **kw)


F32_SUBNORMAL_HALF_STEP = 2.0 ** -150


def assert_f32(rgb, r64):
    """f32 within RTOL of the oracle's f64 colour; NaN where it is NaN.  The two ends
    of the f32 range, by the format alone: an f64 colour beyond it is +-infinity in
    the f32 output (IEEE), and one below 2^-126 (a pow(.., 32) highlight seen through
    thirty refractions is 1e-44) rounds on f32's subnormal grid, whose spacing is
    2^-149 -- the correctly rounded f32 is then up to half a step, 2^-150, away,
    which no relative bound can express."""
    g = rgb.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        r32 = r64.astype(np.float32).astype(np.float64)
        ok = ((np.isnan(r64) & np.isnan(g)) | (np.isinf(r32) & (r32 == g)) |
              (np.abs(g - r64) <= RTOL * np.abs(r64) + F32_SUBNORMAL_HALF_STEP))
    assert ok.all(), f"{(~ok).sum()} colour components beyond rtol {RTOL}"
    assert np.array_equal(np.isnan(g), np.isnan(r64)), "NaN pixels differ"


def assert_exact(rgb, bgr, st, ref):
    assert np.array_equal(bgr, ref["bgr"]), f"{(bgr != ref['bgr']).sum()} BGR bytes differ"
    assert_f32(rgb, ref["rgb64"])
    assert st.rays == ref["counts"]["rays"], (st.rays, ref["counts"]["rays"])
    assert st.shadow_rays == ref["counts"]["shadow_rays"]


def assert_trig_exact(rgb, bgr, st, spec, seed, jitter=1):
    """cos / sin scenes: the device against the oracle's perturbation envelope
    (trig_scenes.Envelope), all of it derived from the reference alone."""
    env = trig_scenes.envelope(spec, seed, jitter)
    env.check_scene()                        # counts and NaN mask fixed, >= 99.99% stable bytes
    ref = env.ref
    assert st.rays == ref["counts"]["rays"], (st.rays, ref["counts"]["rays"])
    assert st.shadow_rays == ref["counts"]["shadow_rays"], (st.shadow_rays, ref["counts"]["shadow_rays"])
    bad = env.stable & (bgr != ref["bgr"])
    assert not bad.any(), f"{bad.sum()} stable BGR bytes differ from the oracle"
    loose = ~env.stable
    if loose.any():
        allowed = (env.bgrs == bgr[None]).any(axis=0)
        assert allowed[loose].all(), f"{(~allowed[loose]).sum()} unstable BGR bytes outside the envelope"
    assert_f32(rgb, ref["rgb64"])
    return env


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


def render_sched(ctx, capfd, spec, G=0, **kw):
    """render() under tuning verbose (and path_group G); -> (rgb, bgr, st, schedule) with the
    schedule the path kernel's verbose line reports: dict(G, T, staged, npix)."""
    with tuning(ctx, verbose=1, path_group=G):
        capfd.readouterr()
        out = render(ctx, spec, **kw)
        err = capfd.readouterr().err
    lines = re.findall(r"rtamd: path G (\d+) T (\d+) staged (\d+) npix (\d+)", err)
    assert len(lines) == 1, err
    g, t, staged, npix = (int(x) for x in lines[0])
    return out + (dict(G=g, T=t, staged=staged, npix=npix),)


def same_render(a, b):
    """Two device renders bitwise identical: f32, BGR and both counts."""
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1], b[1])
    assert (a[2].rays, a[2].shadow_rays) == (b[2].rays, b[2].shadow_rays)


def test_phong_scene_on_path_kernel_is_bit_exact(gpu_ctx):
    spec = scenes.config2(160, 90)
    rgb, bgr, st = render(gpu_ctx, spec, jitter=lr.RT_JITTER_CENTER, algo=lr.RT_ALGO_PATH)
    assert_exact(rgb, bgr, st, ref64.render(spec))


def test_fresnel_scene_on_path_kernel_is_bit_exact(gpu_ctx):
    spec = scenes.config2_fresnel(128, 72)
    rgb, bgr, st = render(gpu_ctx, spec, jitter=lr.RT_JITTER_CENTER, algo=lr.RT_ALGO_PATH)
    assert_exact(rgb, bgr, st, ref64.render(spec))


def test_random_jitter_bit_exact(gpu_ctx):
    spec = scenes.config2(120, 68)
    spec.antialias = 4
    rgb, bgr, st = render(gpu_ctx, spec, seed=11)
    ref = oracle(spec, seed=11)
    assert_exact(rgb, bgr, st, ref)
    # a different seed gives a different image
    _, bgr2, _ = render(gpu_ctx, spec, seed=12)
    assert not np.array_equal(bgr, bgr2)


def _trig_free_stochastic(width, height):
    spec = scenes.stochastic(width, height, antialias=3, samples=1)
    # no IndirectPhong: its bounces use cos/sin
    spec.objects = [o for o in spec.objects if o["material"]["kind"] != "indirect_phong"]
    spec.plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), scenes.phong((0.6, 0.6, 0.6), (0.2, 0.2, 0.2), 16.0, (0.01,) * 3))
    return spec


def test_area_light_and_transparent_bit_exact(gpu_ctx):
    spec = _trig_free_stochastic(96, 64)
    rgb, bgr, st = render(gpu_ctx, spec, seed=5)
    assert_exact(rgb, bgr, st, oracle(spec, seed=5))


@pytest.mark.parametrize("depth", [0, 1, 6])
def test_transparent_depths_centre_jitter(gpu_ctx, depth):
    spec = scenes.SceneSpec(width=80, height=60, antialias=1, max_depth=depth, camera=dict(scenes.DEFAULT_CAMERA),
                            background=(0.2, 0.3, 0.4))
    spec.sphere((0.0, 1.0, -5.0), 1.2, scenes.transparent((0.9, 0.9, 0.9), 64.0, 1.5))
    spec.sphere((0.3, 1.2, -8.0), 1.0, scenes.transparent((0.5, 0.5, 0.5), 16.0, 1.1))
    spec.sphere((-1.5, 0.8, -9.0), 0.8, scenes.phong((0.8, 0.2, 0.2), (0.3,) * 3, 32.0, (0.02, 0.0, 0.0)))
    spec.plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), scenes.phong((0.5, 0.5, 0.5), (0.1,) * 3, 8.0, (0.01,) * 3))
    spec.point_light((-4.0, 6.0, 2.0), (0.9, 0.9, 0.9))
    spec.directional_light((0.2, -1.0, -0.3), (0.2, 0.2, 0.2))
    rgb, bgr, st = render(gpu_ctx, spec, jitter=lr.RT_JITTER_CENTER)
    assert_exact(rgb, bgr, st, ref64.render(spec))


# ---- cos / sin scenes: counts equal, stable bytes equal, the rest inside the oracle's envelope ----

def test_indirect_phong_and_dof_close(gpu_ctx):
    spec = trig_scenes.stochastic_dof()
    rgb, bgr, st = render(gpu_ctx, spec, seed=3)
    env = assert_trig_exact(rgb, bgr, st, spec, 3)
    print(f"stochastic scene (IndirectPhong x2, DoF x2, AreaLight): stable share {env.stable_share:.6f}, "
          f"BGR equal to the unperturbed oracle {float((bgr == env.ref['bgr']).mean()):.6f}")


def test_cornell_keyed_close(gpu_ctx):
    spec = trig_scenes.cornell_small()
    rgb, bgr, st = render(gpu_ctx, spec, seed=1)
    env = assert_trig_exact(rgb, bgr, st, spec, 1)
    print(f"Cornell 64x64x16: stable share {env.stable_share:.6f}, rays {st.rays}")


def test_cornell_matches_out_bmp_statistics(gpu_ctx):
    """The reference's only render: out.bmp, 800x800 with 1024 samples per pixel.
    The device renders the same scene at 200x200 with 1024 samples."""
    spec = cornell_spec(200, 200, antialias=1024)
    _, bgr, st = render(gpu_ctx, spec, seed=2024)
    rms, mx = check_out_bmp_statistics(bgr)
    print(f"out.bmp 8x8 block means: rms {rms:.3f} LSB, max {mx:.3f}; {st.rays} rays in {st.kernel_ms:.1f} ms")


@pytest.mark.parametrize("samples,depth", trig_scenes.CONVEX_CASES)
def test_indirect_phong_convex_bounces(gpu_ctx, samples, depth):
    """Every sample index of an IndirectPhong hit: the per-sample key child(K, i), the
    kFlMore flag, and the frame extension stored before the first child and reloaded
    for each later one (samples 2 and 5), one and three levels deep."""
    spec = trig_scenes.convex_bounce(samples, depth)
    rgb, bgr, st = render(gpu_ctx, spec, seed=40)
    assert_trig_exact(rgb, bgr, st, spec, 40)


def test_indirect_phong_specular_fold_with_exponent_zero(gpu_ctx):
    """IndirectPhong with ks > 0 and exponent 0: the bounce's specular factor
    pow(NaN, 0) is 1 (raytrace.rs:108,115 with C99 pow), so F.g2 folds finite
    colours, after an extension reload too (samples = 2)."""
    build, seed, jitter = trig_scenes.TRIG_SCENES["convex_specular_exp0"]
    spec = build()
    rgb, bgr, st = render(gpu_ctx, spec, seed=seed)
    env = assert_trig_exact(rgb, bgr, st, spec, seed)
    assert not env.nan.any()


def test_dof_lens_samples_average(gpu_ctx):
    """DepthOfFieldCamera with an open aperture and three lens samples: the
    cos / sin lens offset and the `/ ns` average (raytrace.rs:270-276)."""
    spec = trig_scenes.dof_config2()
    rgb, bgr, st = render(gpu_ctx, spec, seed=7)
    assert_trig_exact(rgb, bgr, st, spec, 7)


def test_tiles_and_bands_match_full_frame(gpu_ctx):
    spec = scenes.stochastic(64, 48, antialias=2, samples=1)
    full, fb, _ = render(gpu_ctx, spec, seed=9)
    tile, tb, _ = render(gpu_ctx, spec, seed=9, x0=16, tile_w=32, y0=8, tile_h=24)
    assert np.array_equal(tile, full[8:32, 16:48])
    band, bb, _ = render(gpu_ctx, spec, seed=9, tile_h=16, band=4, band_stride=3, band_phase=1)
    rows = [r for r in range(48) if (r // 4) % 3 == 1]
    assert np.array_equal(band, full[rows])


def test_path_classes_rejected_by_chain_algorithms(gpu_ctx):
    spec = scenes.stochastic(32, 32, antialias=1)
    for algo in (lr.RT_ALGO_WAVEFRONT, lr.RT_ALGO_BRUTE_LDS):
        with pytest.raises(lr.RtError) as e:
            render(gpu_ctx, spec, algo=algo)
        assert e.value.code == lr.RT_E_UNSUPPORTED
    with pytest.raises(lr.RtError) as e:     # random jitter with several samples per pixel
        render(gpu_ctx, scenes.config2(32, 32), algo=lr.RT_ALGO_WAVEFRONT, spp=2)
    assert e.value.code == lr.RT_E_UNSUPPORTED


@pytest.mark.parametrize("algo", [lr.RT_ALGO_WAVEFRONT, lr.RT_ALGO_WAVEFRONT_BRUTE, lr.RT_ALGO_BRUTE_LDS,
                                  lr.RT_ALGO_PATH])
def test_random_jitter_one_sample_on_every_schedule(gpu_ctx, algo):
    """main.rs:51-52 jitters every sample; with one sample per pixel the chain
    schedules (wavefront, megakernel) take the keyed jitter too, and agree with
    the oracle and the path kernel bit for bit (camera tiles widened to whole pixels)."""
    spec = scenes.config3(160, 120, n=300)
    rgb, bgr, st = render(gpu_ctx, spec, seed=21, algo=algo)
    assert_exact(rgb, bgr, st, oracle(spec, seed=21))


@pytest.mark.parametrize("jitter,spp", [(lr.RT_JITTER_CENTER, 1), (lr.RT_JITTER_RANDOM, 3)])
def test_skybox_bit_exact(gpu_ctx, tmp_path, jitter, spp):
    """SkyboxBackground (raytrace.rs:234-256, texture.rs:46-58): camera misses and
    reflections sample the faces; only + - * / and table lookups, so bit-exact."""
    faces = scenes.skybox_faces(size=24, seed=4)
    paths = [str(tmp_path / f"f{k}.ppm") for k in range(6)]
    for p, f in zip(paths, faces):
        scenes.write_ppm(p, f)
    spec = scenes.skybox_scene(paths, 128, 96)
    spec.antialias = spp
    rgb, bgr, st = render(gpu_ctx, spec, jitter=jitter, seed=13)
    assert_exact(rgb, bgr, st, oracle(spec, jitter=jitter, seed=13))
    # the C ABI route (rt_scene_set_skybox) gives the same image as the parsed file
    sc = lr.Scene.deserialize(scenes.skybox_scene(paths, 128, 96).to_text())
    sc2 = lr.Scene.deserialize(scenes.config2(8, 8).to_text())
    gpu_ctx.upload(sc)
    o = lr.render_opts(128, 96, max_depth=spec.max_depth, spp=spp, jitter=jitter, seed=13)
    a = gpu_ctx.render(o)[1]
    txt = scenes.skybox_scene(paths, 128, 96)
    txt.skybox = None
    sc3 = lr.Scene.deserialize(txt.to_text())
    sc3.set_skybox(faces)
    gpu_ctx.upload(sc3)
    assert np.array_equal(gpu_ctx.render(o)[1], a)
    del sc2


def test_cli_renders_the_reference_scene(tmp_path):
    """The main.rs replacement end to end: test_scene.txt in, out.bmp out (header
    bytes as bmp.rs writes them; pixels statistically equal to the reference's)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "rust-raytrace_amd", "raytrace")
    out = str(tmp_path / "out.bmp")
    r = subprocess.run([exe, "--scene", os.path.join(root, "tests", "golden", "test_scene.txt"), "--out", out,
                        "--width", "200", "--height", "200", "--seed", "77"],
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr
    data = open(out, "rb").read()
    hdr, pitch = lr.bmp_header(200, 200)
    assert data[:122] == hdr and len(data) == 122 + pitch * 200
    bgr = np.frombuffer(data[122:], np.uint8).reshape(200, pitch)[:, :600]
    rms, mx = check_out_bmp_statistics(bgr)
    print(f"CLI out.bmp: rms {rms:.3f} LSB vs the reference's out.bmp")


def test_stochastic_edge_cases_bit_exact_without_bounces(gpu_ctx):
    spec = trig_scenes.edge_scene()
    spec.objects = [o for o in spec.objects if o["material"].get("samples", 0) == 0]   # no cos/sin draws
    for depth in (0, 3):
        spec.max_depth = depth
        rgb, bgr, st = render(gpu_ctx, spec, seed=31)
        assert_exact(rgb, bgr, st, oracle(spec, seed=31))


def test_stochastic_edge_cases_close(gpu_ctx):
    spec = trig_scenes.edge_scene()
    rgb, bgr, st = render(gpu_ctx, spec, seed=32)
    env = assert_trig_exact(rgb, bgr, st, spec, 32)
    ref = env.ref
    assert np.isnan(rgb).any() and np.array_equal(np.isnan(rgb), np.isnan(ref["rgb32"]))   # the NaN quirk, same pixels


def test_dof_aperture_zero_equals_pinhole_rays(gpu_ctx):
    """DepthOfFieldCamera with aperture 0: every lens sample starts on the image
    plane point and aims at the focal point (camera.rs:109-122).  The lens offset
    cos(theta) * 0 is exactly +-0 whatever cos returns, so this is bit-exact; the
    three lens samples run the `/ ns` average."""
    spec = trig_scenes.dof_config2(aperture=0.0, samples=3)
    rgb, bgr, st = render(gpu_ctx, spec, jitter=lr.RT_JITTER_CENTER)
    assert_exact(rgb, bgr, st, oracle(spec, jitter=0, seed=7))


# ---- schedules: unstaged tree, several trips of the persistent loop, lanes per pixel ----

@pytest.mark.parametrize("width,height,second_trip", [(512, 288, True), (160, 120, False)])
def test_unstaged_tree_and_second_loop_trip(gpu_ctx, capfd, width, height, second_trip):
    """1000 spheres do not fit the 48 KiB of LDS: path_kernel<0> reads the tree
    through the caches.  At 512x288 the frame has more pixels than the persistent
    grid has work-items, so every work-item takes its stack through a second pixel."""
    spec = scenes.config3(width, height, n=1000)
    rgb, bgr, st, sch = render_sched(gpu_ctx, capfd, spec, seed=21, algo=lr.RT_ALGO_PATH)
    assert sch["staged"] == 0 and sch["G"] == 1 and sch["npix"] == width * height, sch
    assert (sch["npix"] > sch["T"]) == second_trip, sch
    assert_exact(rgb, bgr, st, oracle(spec, seed=21))


_group_refs = {}


@pytest.mark.parametrize("size", [(64, 48), (13, 7)])
@pytest.mark.parametrize("spp", [1, 3, 5, 16])
def test_path_group_forced(gpu_ctx, capfd, spp, size):
    """G lanes of a wave share a pixel and add its AA samples in sample order through
    cross-lane reads: spp below, equal to and no multiple of G (idle lanes feed the
    reads), 64x48 x 64 lanes beyond the grid (a second loop trip with groups), 13x7
    with ragged groups in the last block.  Every G is the oracle's image and, bit for
    bit, G = 1's."""
    spec = scenes.config2(*size)
    spec.antialias = spp
    if (size, spp) not in _group_refs:
        _group_refs[(size, spp)] = oracle(spec, seed=17)
    ref = _group_refs[(size, spp)]
    base = None
    for G in (1, 2, 8, 64):
        rgb, bgr, st, sch = render_sched(gpu_ctx, capfd, spec, G=G, seed=17, algo=lr.RT_ALGO_PATH)
        assert sch["G"] == G and sch["staged"] == 1, sch
        if size == (64, 48) and G == 64:
            assert sch["npix"] * G > sch["T"], sch                 # the second trip, with groups
        if size == (13, 7) and G in (2, 8):
            assert (sch["npix"] * G) % 256 != 0
        assert_exact(rgb, bgr, st, ref)
        if base is None:
            base = (rgb, bgr, st)
        else:
            same_render((rgb, bgr, st), base)


def _cancelling_spheres(spp):
    """Unlit spheres whose ambient colours are +2^100 and -2^100 in turn, over a
    background of order 1: a pixel whose samples see both signs gets the background's
    share only if its samples are added in sample order -- (2^100 + -2^100) + c is c,
    (c + -2^100) + 2^100 is 0 -- so the order of the AA sum shows in the f32 colours
    and not just in the last bit of an f64."""
    spec = scenes.SceneSpec(width=48, height=32, antialias=spp, max_depth=2, camera=dict(scenes.DEFAULT_CAMERA),
                            background=(0.25, 0.5, 0.75))
    big = 2.0 ** 100
    n = 24                      # a lattice finer than the pixels (0.67 units each at this distance), gaps between the spheres
    for i in range(n):
        for j in range(n):
            a = big if (i + j) % 2 == 0 else -big
            spec.sphere((0.4 * (i - 0.5 * n), -0.2 + 0.4 * (j - 0.5 * n), -6.0), 0.18,
                        scenes.phong((0.0,) * 3, (0.0,) * 3, 1.0, (a, 0.5 * a, 0.25 * a)))
    return spec


@pytest.mark.parametrize("spp", [3, 5, 16])
def test_path_group_sum_is_in_sample_order(gpu_ctx, capfd, spp):
    """main.rs:47-55 adds the samples' colours one by one; the lanes of a group must
    add them in that order (and `r / ns` before, `res / aa` after).  Colours that
    cancel make any other order a different image."""
    spec = _cancelling_spheres(spp)
    ref = oracle(spec, seed=19)
    r64 = ref["rgb64"]
    mixed = (np.abs(r64) < 2.0 ** 90).all(axis=2) & (r64 != np.array(spec.background)).any(axis=2)
    assert mixed.sum() >= 15, mixed.sum()             # pixels where +-2^100 samples cancelled: the order-sensitive ones
    base = None
    for G in (1, 2, 8, 64):
        rgb, bgr, st, sch = render_sched(gpu_ctx, capfd, spec, G=G, seed=19, algo=lr.RT_ALGO_PATH)
        assert sch["G"] == G, sch
        assert_exact(rgb, bgr, st, ref)
        if base is None:
            base = (rgb, bgr, st)
        else:
            same_render((rgb, bgr, st), base)


@pytest.mark.parametrize("name", ["stochastic_dof", "cornell_64x64x16"])
def test_stochastic_scenes_across_path_groups(gpu_ctx, capfd, name):
    """Device against device, so libm plays no part: 1, 4 and 64 lanes per pixel give
    the same bits; each is also inside the oracle's envelope."""
    build, seed, jitter = trig_scenes.TRIG_SCENES[name]
    spec = build()
    base = None
    for G in (1, 4, 64):
        rgb, bgr, st, sch = render_sched(gpu_ctx, capfd, spec, G=G, seed=seed)
        assert sch["G"] == G, sch
        assert_trig_exact(rgb, bgr, st, spec, seed, jitter)
        if base is None:
            base = (rgb, bgr, st)
        else:
            same_render((rgb, bgr, st), base)


def _branching_spheres(depth):
    spec = scenes.config3(96, 72)
    spec.max_depth = depth
    spec.antialias = 2
    rest = 0
    for i, o in enumerate(spec.objects):
        m = o["material"]
        ior = 1.3 + 0.01 * (i % 20)
        if i % 3 == 0:
            o["material"] = scenes.transparent(m["specular"], m["exponent"], ior)
        else:
            if rest % 3 == 0:
                o["material"] = scenes.fresnel(m["diffuse"], m["specular"], m["exponent"], m["ambient"], ior)
            rest += 1
    return spec


@pytest.mark.parametrize("depth", [6, 12])
def test_transparent_and_fresnel_in_a_large_tree(gpu_ctx, capfd, depth):
    """A third of 1000 spheres Transparent, a third of the rest Fresnel: refraction
    rays start inside their sphere (the shadow and child queries' `hint`), in the
    unstaged tree, reflection + refraction children down to depth 12."""
    spec = _branching_spheres(depth)
    rgb, bgr, st, sch = render_sched(gpu_ctx, capfd, spec, seed=23)
    assert sch["staged"] == 0, sch
    assert_exact(rgb, bgr, st, oracle(spec, seed=23))


@pytest.mark.parametrize("ior", [1.0, 0.7, 2.4])
def test_nested_transparent_spheres_camera_inside(gpu_ctx, ior):
    """A Transparent sphere inside a Transparent sphere, the camera inside the outer
    one: ior 1 (r0 = 0, rays pass straight), ior < 1, and dense glass (total internal
    reflection), to the deepest recursion the ABI allows."""
    spec = scenes.SceneSpec(width=48, height=36, antialias=1, max_depth=lr.RT_MAX_DEPTH_LIMIT,
                            camera=dict(scenes.DEFAULT_CAMERA), background=(0.2, 0.3, 0.4))
    spec.sphere((0.0, 3.0, 8.0), 5.0, scenes.transparent((0.3, 0.3, 0.3), 32.0, ior))
    spec.sphere((0.0, 2.5, 5.5), 1.2, scenes.transparent((0.3, 0.25, 0.2), 16.0, ior))
    spec.sphere((-2.0, 1.0, -6.0), 1.0, scenes.phong((0.8, 0.2, 0.2), (0.3,) * 3, 32.0, (0.02, 0.0, 0.0)))
    spec.plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), scenes.phong((0.5, 0.5, 0.5), (0.1,) * 3, 8.0, (0.01,) * 3))
    spec.point_light((-4.0, 9.0, 6.0), (0.9, 0.9, 0.9))
    spec.directional_light((0.2, -1.0, -0.3), (0.2, 0.2, 0.2))
    ref = ref64.render(spec)
    assert 48 * 36 < ref["counts"]["rays"] < 2_000_000, ref["counts"]       # branching stays bounded
    rgb, bgr, st = render(gpu_ctx, spec, jitter=lr.RT_JITTER_CENTER)
    assert_exact(rgb, bgr, st, ref)


@pytest.mark.parametrize("scene", ["nan_plane_scene", "axis_tie_scene", "coincident_scene", "extreme_magnitudes_scene"])
def test_adversarial_scenes_on_path_kernel(gpu_ctx, scene):
    """The wavefront tests' adversarial scenes (NaN plane hits, exact-axis rays and
    ties across leaves, coincident objects, operands far from unit magnitude)
    through the path kernel's own nearest-hit and shadow queries."""
    spec = getattr(adversarial_scenes, scene)()
    rgb, bgr, st = render(gpu_ctx, spec, jitter=lr.RT_JITTER_CENTER, algo=lr.RT_ALGO_PATH)
    assert_exact(rgb, bgr, st, ref64.render(spec))


@pytest.mark.parametrize("G", [1, 8])
def test_tiles_bands_and_pitch_match_oracle(gpu_ctx, capfd, G):
    """Tile offsets, row bands and a padded BGR pitch on the path kernel, one and
    eight lanes per pixel: bytes, zero padding, f32 and counts are the oracle's."""
    spec = _trig_free_stochastic(67, 41)
    for (x0, tw, y0, th, band, stride, phase) in [(0, 67, 0, 41, 1, 1, 0), (5, 17, 3, 13, 1, 1, 0),
                                                   (0, 67, 0, 12, 4, 3, 1), (10, 50, 1, 15, 5, 2, 1)]:
        tile = dict(x0=x0, tile_w=tw, y0=y0, tile_h=th, band=band, band_stride=stride, band_phase=phase)
        rgb, bgr, st, sch = render_sched(gpu_ctx, capfd, spec, G=G, seed=5, bgr_pitch=3 * tw + 5, **tile)
        assert sch["G"] == G and sch["npix"] == tw * th, sch
        ref = oracle(spec, seed=5, **tile)
        assert bgr.shape == (th, 3 * tw + 5)
        assert (bgr[:, 3 * tw:] == 0).all()           # BMP row padding (main.rs:42)
        assert_exact(rgb, np.ascontiguousarray(bgr[:, :3 * tw]), st, ref)


def _edge_faces():
    """Skybox faces of 1x1, 2x2 and non-square 5x3 / 3x5 texels, no texel black."""
    rng = scenes.SplitMix64(9)
    faces = []
    for h, w in [(1, 1), (2, 2), (3, 5), (5, 3), (2, 2), (1, 1)]:
        faces.append(np.array([1 + rng.next() % 255 for _ in range(h * w * 3)], np.uint8).reshape(h, w, 3))
    return faces


@pytest.mark.parametrize("jitter,spp", [(lr.RT_JITTER_CENTER, 1), (lr.RT_JITTER_RANDOM, 3)])
def test_skybox_edges(gpu_ctx, tmp_path, jitter, spp):
    """One-texel, 2x2 and non-square faces, and a frame (33x16, camera on the axes)
    whose columns 8 and 24 look along |dx| == |dz| exactly: no axis dominates and
    the background is BLACK (raytrace.rs:234-256)."""
    paths = [str(tmp_path / f"e{k}.ppm") for k in range(6)]
    for p, f in zip(paths, _edge_faces()):
        scenes.write_ppm(p, f)
    spec = scenes.SceneSpec(width=33, height=16, antialias=spp, max_depth=4, skybox=paths,
                            camera={"ctor": "new", "position": (0, 0, 0), "look": (0, 0, -1), "up": (0, 1, 0),
                                    "im_dist": 1.0})
    spec.sphere((0.0, 0.0, -6.0), 1.0, scenes.phong((0.1, 0.1, 0.1), (0.8, 0.8, 0.8), 64.0, (0.0, 0.0, 0.0)))
    spec.sphere((0.45, 0.3, -3.0), 0.3, scenes.transparent((0.9, 0.9, 0.9), 64.0, 1.4))
    spec.point_light((-10.0, 10.0, 5.0), (0.8, 0.8, 0.8))
    ref = oracle(spec, jitter=jitter, seed=13)
    if jitter == lr.RT_JITTER_CENTER:
        black = (ref["rgb64"] == 0.0).all(axis=2)
        assert black[:, 8].all() and black[:, 24].all() and black.sum() >= spec.height
    rgb, bgr, st = render(gpu_ctx, spec, jitter=jitter, seed=13)
    assert_exact(rgb, bgr, st, ref)
    # the same faces behind the default camera's tilted view
    spec2 = scenes.skybox_scene(paths, 40, 30)
    spec2.antialias = spp
    rgb, bgr, st = render(gpu_ctx, spec2, jitter=jitter, seed=13)
    assert_exact(rgb, bgr, st, oracle(spec2, jitter=jitter, seed=13))
