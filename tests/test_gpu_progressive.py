"""Progressive rendering: rt_render_accumulate adds sample ranges to a device-resident f64
accumulator, rt_accum_resolve* gives the image of the samples so far (main.rs:47-56 split over calls).

The contract: accumulating samples [0, k) and then [k, n) is, bit for bit, the one-shot render with
spp = n (the oracle's jitter=1, rng=1 render), on the path kernel, on the wavefront passes and on a
mixture of both, and a resolve after k samples is the oracle's spp = k render.  The sums continue the
reference's `res = res + s_a` one sample at a time in sample order; the cancelling scene (ambient
+-2^100 over a background of order 1) turns any other order across the call boundary into another
f32 image (tests/test_progressive_oracle.py shows, from the oracle alone, that its splits do).

The oracle's renders are computed once per (scene, spp, seed, tile) and left unchanged.
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
PATH, AA, AUTO = lr.RT_ALGO_PATH, lr.RT_ALGO_WAVEFRONT_AA, lr.RT_ALGO_AUTO
ACC_LINE = re.compile(r"rtamd: accumulate samples \[(\d+), (\d+)\) (path|passes)")
AA_LINE = re.compile(r"rtamd: aa passes (\d+), chunks (\d+) x (\d+) rows")
PATH_LINE = re.compile(r"rtamd: path G (\d+) T (\d+) staged (\d+) npix (\d+)")
GROWN = re.compile(r"rtamd: lane working set grown")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rust-raytrace_amd", "raytrace")

_refs = {}


def oracle(key, spec, spp, seed, **tile):
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


def opts(spec, seed, spp=1, algo=AUTO, jitter=lr.RT_JITTER_RANDOM, **kw):
    return lr.render_opts(spec.width, spec.height, max_depth=spec.max_depth, spp=spp, algo=algo, jitter=jitter,
                          seed=seed, **kw)


def assert_f32(rgb, r64):
    g = rgb.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        r32 = r64.astype(np.float32).astype(np.float64)
        ok = ((np.isnan(r64) & np.isnan(g)) | (np.isinf(r32) & (r32 == g)) |
              (np.abs(g - r64) <= RTOL * np.abs(r64) + F32_SUBNORMAL_HALF_STEP))
    assert ok.all(), f"{(~ok).sum()} colour components beyond rtol {RTOL}"
    assert np.array_equal(np.isnan(g), np.isnan(r64)), "NaN pixels differ"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def add(ctx, capfd, acc, n, algo, **kw):
    """One rt_render_accumulate under tuning verbose; -> (its statistics, its stderr).  The verbose line must
    name the range and the schedule that ran."""
    s0 = acc.samples
    with tuning(ctx, verbose=1):
        capfd.readouterr()
        acc.add(n, algo, **kw)
        st = ctx.stats()
        err = capfd.readouterr().err
    assert acc.samples == s0 + n
    lines = ACC_LINE.findall(err)
    assert len(lines) == 1 and (int(lines[0][0]), int(lines[0][1])) == (s0, s0 + n), err
    if algo != AUTO:
        assert lines[0][2] == ("path" if algo == PATH else "passes"), err
    if lines[0][2] == "path":
        assert PATH_LINE.search(err) and not AA_LINE.search(err), err
    else:
        m = AA_LINE.findall(err)
        assert len(m) == 1 and int(m[0][0]) == n and not PATH_LINE.search(err), err
    assert st.traced_rays == st.rays
    return st, err


def accumulate(ctx, capfd, spec, seed, split, algos, tune=None, upload=True, **okw):
    """A fresh accumulator, the split's calls, one host resolve; -> (rgb, bgr, [statistics per call], acc)."""
    if upload:
        with tuning(ctx, **{k: v for k, v in (tune or {}).items() if k == "light_grids"}):
            ctx.upload(lr.Scene.deserialize(spec.to_text()))
    acc = ctx.accumulator(opts(spec, seed, **okw))
    sts = []
    with tuning(ctx, **(tune or {})):
        for n, algo in zip(split, algos):
            sts.append(add(ctx, capfd, acc, n, algo)[0])
        rgb, bgr = acc.resolve()
    return rgb, bgr, sts, acc


def check(rgb, bgr, sts, ref):
    assert np.array_equal(bgr, ref["bgr"]), f"{(bgr != ref['bgr']).sum()} BGR bytes differ"
    assert_f32(rgb, ref["rgb64"])
    assert sum(s.rays for s in sts) == ref["counts"]["rays"]
    assert sum(s.shadow_rays for s in sts) == ref["counts"]["shadow_rays"]


# ---- split equals one-shot and oracle ----

SPLITS = [(5,), (2, 3), (1, 1, 1, 1, 1), (1, 4)]
SPLIT_CASES = [(s, a) for s in SPLITS for a in ("path", "passes")] + \
              [(s, a) for s in ((2, 3), (3, 2)) for a in ("path_then_passes", "passes_then_path")]
_oneshot = {}


@pytest.mark.parametrize("split,algo", SPLIT_CASES, ids=lambda v: "+".join(map(str, v)) if isinstance(v, tuple) else v)
def test_split_equals_one_shot_and_oracle(gpu_ctx, capfd, split, algo):
    spec = scenes.config3(96, 64, n=300)
    ref = oracle("c3_96", spec, 5, 7)
    algos = {"path": [PATH] * len(split), "passes": [AA] * len(split), "path_then_passes": [PATH, AA],
             "passes_then_path": [AA, PATH]}[algo]
    rgb, bgr, sts, acc = accumulate(gpu_ctx, capfd, spec, 7, split, algos)
    acc.close()
    check(rgb, bgr, sts, ref)
    if "one" not in _oneshot:
        _oneshot["one"] = gpu_ctx.render(opts(spec, 7, spp=5, algo=PATH))
    one = _oneshot["one"]
    assert np.array_equal(bits(rgb), bits(one[0])) and np.array_equal(bgr, one[1])
    assert all(s.pixels == 96 * 64 for s in sts)
    assert all((s.chunks == 0) == (a == PATH) for s, a in zip(sts, algos))


def test_fresnel_planes_one_plus_three(gpu_ctx, capfd):
    spec = scenes.config2_fresnel(80, 45)
    ref = oracle("c2f", spec, 4, 11)
    for algos in ([PATH, PATH], [AA, AA]):
        rgb, bgr, sts, acc = accumulate(gpu_ctx, capfd, spec, 11, (1, 3), algos)
        acc.close()
        check(rgb, bgr, sts, ref)


# ---- prefix resolves ----

@pytest.mark.parametrize("algo", [PATH, AA])
def test_prefix_resolves(gpu_ctx, capfd, algo):
    spec = scenes.config3(96, 64, n=300)
    r2, r5 = oracle("c3_96", spec, 2, 7), oracle("c3_96", spec, 5, 7)
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    with gpu_ctx.accumulator(opts(spec, 7)) as acc:
        st2, _ = add(gpu_ctx, capfd, acc, 2, algo)
        a = acc.resolve()
        b = acc.resolve()                                   # non-destructive: twice the same bits
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
        check(a[0], a[1], [st2], r2)
        assert acc.samples == 2
        st3, _ = add(gpu_ctx, capfd, acc, 3, algo)
        c = acc.resolve()
        check(c[0], c[1], [st2, st3], r5)
        # n == 0 is RT_OK and renders nothing
        before = gpu_ctx.stats()
        acc.add(0, algo)
        after = gpu_ctx.stats()
        assert acc.samples == 5 and (before.rays, before.pixels) == (after.rays, after.pixels)


# ---- order across the call boundary ----

def cancelling_spheres():
    """test_gpu_aa.py's cancelling scene: unlit Phong spheres whose ambient colours are +2^100 and
    -2^100 in turn over a background of order 1."""
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


ORDER_SPLITS = [(1, 4), (2, 3), (3, 2), (3, 5, 8)]


@pytest.mark.parametrize("compose", [0, 1])
@pytest.mark.parametrize("split", ORDER_SPLITS, ids=lambda s: "+".join(map(str, s)))
def test_order_across_the_boundary_on_the_passes(gpu_ctx, capfd, split, compose):
    spec = cancelling_spheres()
    ref = oracle("cancel", spec, sum(split), 19)
    rgb, bgr, sts, acc = accumulate(gpu_ctx, capfd, spec, 19, split, [AA] * len(split), tune=dict(compose=compose))
    acc.close()
    check(rgb, bgr, sts, ref)
    assert np.array_equal(bits(rgb), bits(ref["rgb32"]))          # any other order: another f32 image


@pytest.mark.parametrize("G", [1, 2, 8, 64])
@pytest.mark.parametrize("split", ORDER_SPLITS, ids=lambda s: "+".join(map(str, s)))
def test_order_across_the_boundary_on_the_path_kernel(gpu_ctx, capfd, split, G):
    """n below G, n no multiple of G: idle lanes feed the cross-lane reads, the sum continues from the loaded one."""
    spec = cancelling_spheres()
    ref = oracle("cancel", spec, sum(split), 19)
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    with tuning(gpu_ctx, path_group=G), gpu_ctx.accumulator(opts(spec, 19)) as acc:
        sts = []
        for n in split:
            st, err = add(gpu_ctx, capfd, acc, n, PATH)
            assert int(PATH_LINE.search(err).group(1)) == G, err
            sts.append(st)
        rgb, bgr = acc.resolve()
    check(rgb, bgr, sts, ref)
    assert np.array_equal(bits(rgb), bits(ref["rgb32"]))


def test_second_trip_of_the_persistent_loop_with_groups(gpu_ctx, capfd):
    """64x48 pixels x 64 lanes are more work-items than the persistent grid has: every group takes a second
    pixel (test_gpu_path.py's way of forcing it), loading and storing that pixel's sum."""
    spec = scenes.config2(64, 48)
    ref = oracle("c2_64", spec, 5, 17)
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    with tuning(gpu_ctx, path_group=64), gpu_ctx.accumulator(opts(spec, 17)) as acc:
        sts = []
        for n in (2, 3):
            st, err = add(gpu_ctx, capfd, acc, n, PATH)
            m = PATH_LINE.search(err)
            assert int(m.group(1)) == 64 and int(m.group(4)) * 64 > int(m.group(2)), err
            sts.append(st)
        rgb, bgr = acc.resolve()
    check(rgb, bgr, sts, ref)
    assert np.array_equal(bits(rgb), bits(ref["rgb32"]))


# ---- -0.0 and NaN ----

@pytest.mark.parametrize("algo", [PATH, AA])
def test_negative_zero_and_nan_samples(gpu_ctx, capfd, algo):
    spec = adversarial_scenes.tiny(width=24, height=16)
    spec.background = (-0.0, 0.0, -0.0)
    spec.sphere((0.0, 0.0, -4.0), 1.0, scenes.phong((0.0,) * 3, (0.0,) * 3, 1.0, (0.5, 0.25, -0.0)))
    ref = oracle("neg_zero", spec, 3, 29)
    assert (ref["rgb64"] == 0.0).any() and not np.signbit(ref["rgb64"]).any()
    rgb, bgr, sts, acc = accumulate(gpu_ctx, capfd, spec, 29, (1, 2), [algo] * 2)
    check(rgb, bgr, sts, ref)
    assert np.array_equal(bits(rgb), bits(ref["rgb32"])) and not np.signbit(rgb).any()
    # a single -0.0 sample too: the first sample is 0.0 + s_0
    acc.reset()
    st, _ = add(gpu_ctx, capfd, acc, 1, algo)
    one = acc.resolve()
    acc.close()
    assert not np.signbit(one[0]).any()
    nan = adversarial_scenes.tiny(width=24, height=16)
    nan.background = (-0.0, 0.0, -0.0)
    nan.sphere((0.0, 0.0, -4.0), 1.0, scenes.phong((0.0,) * 3, (0.0,) * 3, 1.0, (0.5, 0.25, -0.0)))
    nan.plane((0, 0, 0), (0, 0, 0), scenes.phong((0.1, 0.2, 0.3), (0.2, 0.2, 0.2), 4.0, (0, 0, 1)))
    nan.point_light((3, 3, 3), (1, 1, 1))
    ref = oracle("nan_plane_all", nan, 3, 29)
    assert np.isnan(ref["rgb64"]).all()
    rgb, bgr, sts, acc = accumulate(gpu_ctx, capfd, nan, 29, (1, 2), [algo] * 2)
    check(rgb, bgr, sts, ref)
    assert np.isnan(rgb).all()
    # the accumulator is full of NaN now.  Another scene, a reset, one sample: the oracle's spp = 1 render,
    # so the first sample stores without reading whatever an earlier render left
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    acc.reset()
    st, _ = add(gpu_ctx, capfd, acc, 1, algo)
    rgb, bgr = acc.resolve()
    acc.close()
    ref1 = oracle("neg_zero", spec, 1, 29)
    check(rgb, bgr, [st], ref1)
    assert np.array_equal(bits(rgb), bits(ref1["rgb32"]))


# ---- path-only classes ----

def test_path_only_classes(gpu_ctx, capfd):
    """test_gpu_path.py's bit-exact Transparent + AreaLight scene (no trig): 4 samples as 1 + 3."""
    spec = scenes.stochastic(48, 32, antialias=3, samples=1)
    spec.objects = [o for o in spec.objects if o["material"]["kind"] != "indirect_phong"]
    spec.plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), scenes.phong((0.6, 0.6, 0.6), (0.2, 0.2, 0.2), 16.0, (0.01,) * 3))
    ref = oracle("stoch", spec, 4, 5)
    for algos in ([PATH, PATH], [AUTO, AUTO]):
        rgb, bgr, sts, acc = accumulate(gpu_ctx, capfd, spec, 5, (1, 3), algos)
        check(rgb, bgr, sts, ref)
        assert np.array_equal(bits(rgb), bits(ref["rgb32"]))
    before = gpu_ctx.stats()
    with pytest.raises(lr.RtError) as e:
        acc.add(1, AA)
    assert e.value.code == lr.RT_E_UNSUPPORTED and "RT_ALGO_PATH" in str(e.value)
    after = gpu_ctx.stats()
    assert acc.samples == 4 and (before.rays, before.shadow_rays) == (after.rays, after.shadow_rays)
    acc.close()


def test_auto_follows_aa_wavefront(gpu_ctx, capfd):
    spec = scenes.config3(96, 64, n=300)
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    with gpu_ctx.accumulator(opts(spec, 7)) as acc:
        _, err = add(gpu_ctx, capfd, acc, 1, AUTO)
        assert ACC_LINE.search(err).group(3) == "path"
        with tuning(gpu_ctx, aa_wavefront=1):
            _, err = add(gpu_ctx, capfd, acc, 1, AUTO)          # one sample: still the passes, never a shortcut
        assert ACC_LINE.search(err).group(3) == "passes"
        rgb, bgr = acc.resolve()
    ref = oracle("c3_96", spec, 2, 7)
    assert np.array_equal(bgr, ref["bgr"])


# ---- tree beyond LDS ----

def test_config4_tree_beyond_lds(gpu_ctx, capfd):
    spec = scenes.config4(64, 48)
    rgb, bgr, sts, acc = accumulate(gpu_ctx, capfd, spec, 5, (1, 1), [AA, AA])
    acc.close()
    check(rgb, bgr, sts, oracle("c4", spec, 2, 5))


# ---- geometry ----

def _hip():
    hip = lr.lib          # the HIP runtime librtamd.so is linked against (test_gpu_aa.py)
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    return hip


@pytest.mark.parametrize("algo", [PATH, AA])
def test_tile_offsets_bands_and_pitch(gpu_ctx, capfd, algo):
    spec = scenes.config3(96, 64, n=300)
    full = oracle("c3_96", spec, 3, 7)
    tile = dict(x0=5, tile_w=17, y0=3, tile_h=13)
    tref = oracle("c3_96", spec, 3, 7, **tile)
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    hip = _hip()
    with gpu_ctx.accumulator(opts(spec, 7, **tile)) as acc:
        sts = [add(gpu_ctx, capfd, acc, n, algo)[0] for n in (1, 2)]
        assert all(s.pixels == 17 * 13 for s in sts)
        for pitch in (3 * 17 + 5, 3 * 17 + 2):             # dword stores / byte stores
            rgb, bgr = acc.resolve(pitch=pitch)
            check(rgb, bgr[:, :51], sts, tref)
            assert np.array_equal(bgr[:, :51], full["bgr"][3:16, 15:66])
            assert (bgr[:, 51:] == 0).all()                # the host resolve writes the padding as zero
            # the device resolve leaves it, and the bytes around the rows
            guard = 256
            n_bgr = guard + 13 * pitch + guard
            h_bgr = np.full(n_bgr, 0xCD, np.uint8)
            h_rgb = np.full(13 * 17 * 3, np.nan, np.float32)
            d_bgr, d_rgb = ctypes.c_void_p(), ctypes.c_void_p()
            assert hip.hipMalloc(ctypes.byref(d_bgr), n_bgr) == 0 and hip.hipMalloc(ctypes.byref(d_rgb), h_rgb.nbytes) == 0
            try:
                assert hip.hipMemcpy(d_bgr, h_bgr.ctypes.data, n_bgr, 1) == 0
                assert hip.hipMemcpy(d_rgb, h_rgb.ctypes.data, h_rgb.nbytes, 1) == 0
                acc.resolve_device(d_rgb.value, d_bgr.value + guard, pitch=pitch)
                gpu_ctx.stats()                            # synchronises with the context's stream
                assert hip.hipMemcpy(h_bgr.ctypes.data, d_bgr, n_bgr, 2) == 0
                assert hip.hipMemcpy(h_rgb.ctypes.data, d_rgb, h_rgb.nbytes, 2) == 0
            finally:
                hip.hipFree(d_bgr)
                hip.hipFree(d_rgb)
            rows = h_bgr[guard:guard + 13 * pitch].reshape(13, pitch)
            assert np.array_equal(rows[:, :51], tref["bgr"])
            assert (rows[:, 51:] == 0xCD).all(), "row padding written"
            assert (h_bgr[:guard] == 0xCD).all() and (h_bgr[guard + 13 * pitch:] == 0xCD).all(), "guard bytes written"
            assert np.array_equal(bits(h_rgb.reshape(13, 17, 3)), bits(rgb))
    # row bands with band_stride 2: the rows of the full frame
    with gpu_ctx.accumulator(opts(spec, 7, tile_h=24, band=4, band_stride=2, band_phase=1)) as acc:
        for n in (2, 1):
            add(gpu_ctx, capfd, acc, n, algo)
        rgb, bgr = acc.resolve()
    rows = [r for r in range(64) if (r // 4) % 2 == 1][:24]
    assert np.array_equal(bgr, full["bgr"][rows])
    assert np.array_equal(bits(rgb), bits(full["rgb32"][rows]))


def test_chunked_passes_equal_one_chunk(gpu_ctx, capfd):
    spec = scenes.config3(128, 96)
    ref = oracle("c3_128", spec, 3, 31)
    base = accumulate(gpu_ctx, capfd, spec, 31, (1, 2), [AA, AA])
    base[3].close()
    check(base[0], base[1], base[2], ref)
    assert all(s.chunks == 1 for s in base[2])
    for tune in (dict(chunk_pixels=128 * 32), dict(chunk_pixels=128 * 32, lanes=2, compose=1)):
        out = accumulate(gpu_ctx, capfd, spec, 31, (1, 2), [AA, AA], tune=tune, upload=False)
        out[3].close()
        assert all(s.chunks == 3 for s in out[2]), [s.chunks for s in out[2]]
        check(out[0], out[1], out[2], ref)
        assert np.array_equal(bits(out[0]), bits(base[0])) and np.array_equal(out[1], base[1])


def test_resolve_is_timed_as_compose(gpu_ctx, capfd):
    """RT_TIME_KERNELS on the accumulate: its passes' launches and the resolve after it (RT_KF_COMPOSE) are timed;
    the per-chunk accum_resolve never runs."""
    spec = scenes.config3(96, 64, n=300)
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    for compose in (0, 1):
        with tuning(gpu_ctx, compose=compose), gpu_ctx.accumulator(opts(spec, 7)) as acc:
            gpu_ctx.kernel_times()
            add(gpu_ctx, capfd, acc, 2, AA, flags=lr.RT_TIME_KERNELS)
            kt = gpu_ctx.kernel_times()
            assert kt["camera"][1] == 2 and kt["tally"][1] == 2 and kt["compose"][1] == 2 * compose, kt
            acc.resolve()
            assert gpu_ctx.kernel_times()["compose"][1] == 1
            add(gpu_ctx, capfd, acc, 1, PATH)               # an untimed call: the resolve after it is not timed
            gpu_ctx.kernel_times()
            acc.resolve()
            assert gpu_ctx.kernel_times()["compose"][1] == 0


# ---- checkpoint ----

@pytest.mark.parametrize("through_file", [False, True])
def test_download_upload_continues_in_a_fresh_context(gpu_ctx, capfd, tmp_path, through_file):
    spec = scenes.config3(96, 64, n=300)
    ref = oracle("c3_96", spec, 5, 7)
    text = spec.to_text()
    gpu_ctx.upload(lr.Scene.deserialize(text))
    o = opts(spec, 7)
    with gpu_ctx.accumulator(o) as acc:
        add(gpu_ctx, capfd, acc, 2, AA)
        sums, n = acc.download()
        assert n == 2 and sums.shape == (64, 96, 3)
        add(gpu_ctx, capfd, acc, 3, PATH)
        whole = acc.resolve()
    if through_file:
        path = str(tmp_path / "render.ckpt")
        lr.checkpoint_write(path, o, lr.scene_hash(text), n, sums)
        o2, h, n2, sums2 = lr.checkpoint_read(path)
        assert (h, n2) == (lr.scene_hash(text), 2) and np.array_equal(sums2.view(np.uint64), sums.view(np.uint64))
        for f in ("width", "height", "x0", "tile_w", "y0", "tile_h", "band", "band_stride", "band_phase", "max_depth",
                  "jitter", "seed"):
            assert getattr(o2, f) == getattr(o, f) or (f in ("band", "band_stride") and getattr(o2, f) in (0, 1)), f
        assert lr.checkpoint_read(path, header_only=True)[2] == 2
        with pytest.raises(lr.RtError) as e:
            lr.checkpoint_read(str(tmp_path / "missing.ckpt"))
        assert e.value.code == lr.RT_E_IO
        sums, n = sums2, n2
    with lr.Context(0) as ctx:
        ctx.upload(lr.Scene.deserialize(text))
        with ctx.accumulator(o) as acc:
            acc.upload(sums, n)
            assert acc.samples == 2
            add(ctx, capfd, acc, 3, PATH)
            rgb, bgr = acc.resolve()
    assert np.array_equal(bits(rgb), bits(whole[0])) and np.array_equal(bgr, whole[1])
    assert np.array_equal(bgr, ref["bgr"])
    assert_f32(rgb, ref["rgb64"])


# ---- refusals ----

def test_refusals(gpu_ctx, capfd):
    spec = scenes.config3(96, 64, n=300)
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    acc = gpu_ctx.accumulator(opts(spec, 7))
    with pytest.raises(lr.RtError) as e:
        acc.resolve()
    assert e.value.code == lr.RT_E_INVALID                    # no samples yet
    st0, _ = add(gpu_ctx, capfd, acc, 1, PATH)

    def refused(code, fn):
        with pytest.raises(lr.RtError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        st = gpu_ctx.stats()                                 # a refused call is no render
        assert (st.rays, st.shadow_rays, st.pixels, st.chunks) == (st0.rays, st0.shadow_rays, st0.pixels, st0.chunks)
        assert acc.samples == 1

    for algo in (lr.RT_ALGO_BRUTE_LDS, lr.RT_ALGO_BRUTE_GLOBAL, lr.RT_ALGO_WAVEFRONT, lr.RT_ALGO_WAVEFRONT_BRUTE):
        refused(lr.RT_E_UNSUPPORTED, lambda: acc.add(1, algo))
    refused(lr.RT_E_INVALID, lambda: acc.add(1, 7))
    for flags in (lr.RT_OUT_RGB_F32, lr.RT_OUT_BGR_U8, lr.RT_OUT_FRAME_ROWS, 32, lr.RT_COUNT_WORK | lr.RT_OUT_BGR_U8):
        refused(lr.RT_E_INVALID, lambda: acc.add(1, PATH, flags=flags))
    refused(lr.RT_E_INVALID, lambda: acc.add(2 ** 31, PATH))  # 1 + 2^31 samples
    refused(lr.RT_E_INVALID, lambda: acc.upload(np.zeros(96 * 64 * 3 - 1), 1))
    refused(lr.RT_E_INVALID, lambda: acc.upload(np.zeros(96 * 64 * 3 + 3), 1))
    refused(lr.RT_E_INVALID, lambda: acc.download(cap=96 * 64 * 3 - 1))
    refused(lr.RT_E_INVALID, lambda: acc.resolve(pitch=3 * 96 - 1))
    # the allowed flags work
    st, _ = add(gpu_ctx, capfd, acc, 1, AA, flags=lr.RT_COUNT_WORK | lr.RT_TIME_KERNELS)
    assert st.sphere_tests > 0
    acc.reset()
    st0, _ = add(gpu_ctx, capfd, acc, 1, PATH)
    # another scene: every use is refused until reset()
    spec2 = scenes.config2(96, 64)
    spec2.max_depth = spec.max_depth                        # the accumulator's bound depth
    gpu_ctx.upload(lr.Scene.deserialize(spec2.to_text()))
    for fn in (lambda: acc.add(1, PATH), acc.resolve, acc.download, lambda: acc.upload(np.zeros(96 * 64 * 3), 1),
               lambda: acc.resolve_device(0, 0)):
        with pytest.raises(lr.RtError) as e:
            fn()
        assert e.value.code == lr.RT_E_INVALID and "rt_accum_reset" in str(e.value)
    assert acc.samples == 1
    acc.reset()
    assert acc.samples == 0
    st, _ = add(gpu_ctx, capfd, acc, 2, PATH)
    rgb, bgr = acc.resolve()
    check(rgb, bgr, [st], oracle("c2_96", spec2, 2, 7))
    acc.close()
    # an accumulator is its context's
    with lr.Context(0) as other:
        other.upload(lr.Scene.deserialize(spec.to_text()))
        with other.accumulator(opts(spec, 7)) as theirs:
            assert lr.lib.rt_render_accumulate(gpu_ctx._h, theirs._h, 1, PATH, 0, None) == lr.RT_E_INVALID


# ---- lifecycle ----

def test_reserved_accumulate_allocates_nothing(capfd):
    spec = scenes.config3(96, 64, n=300)
    ref = oracle("c3_96", spec, 3, 7)
    with lr.Context(0, tuning={"verbose": 1}) as ctx:
        ctx.upload(lr.Scene.deserialize(spec.to_text()))
        ctx.reserve(opts(spec, 7, spp=3, algo=AA))
        assert GROWN.search(capfd.readouterr().err)
        with ctx.accumulator(opts(spec, 7)) as acc:
            capfd.readouterr()
            acc.add(3, AA)
            st = ctx.stats()
            err = capfd.readouterr().err
            assert ACC_LINE.search(err) and not GROWN.search(err) and "released" not in err, err
            rgb, bgr = acc.resolve()
        check(rgb, bgr, [st], ref)


def test_statistics_read_late(capfd):
    """After another accumulator's call and a set_tuning, the statistics are the last call's."""
    spec = scenes.config3(96, 64, n=300)
    r1, r2 = oracle("c3_96", spec, 1, 7), oracle("c3_96", spec, 2, 7)
    with lr.Context(0) as ctx:
        ctx.upload(lr.Scene.deserialize(spec.to_text()))
        a, b = ctx.accumulator(opts(spec, 7)), ctx.accumulator(opts(spec, 7))
        a.add(2, AA)
        st = ctx.stats()
        assert (st.rays, st.shadow_rays, st.chunks) == (r2["counts"]["rays"], r2["counts"]["shadow_rays"], 1)
        a.add(1, PATH)
        b.add(1, AA)
        ctx.set_tuning("compose", 1)
        ctx.set_tuning("chunk_pixels", 96 * 16)
        for _ in range(2):
            st = ctx.stats()
            assert (st.rays, st.shadow_rays, st.pixels, st.chunks) == \
                (r1["counts"]["rays"], r1["counts"]["shadow_rays"], 96 * 64, 1)
        assert (a.samples, b.samples) == (3, 1)
        rgb, bgr = b.resolve()
        assert np.array_equal(bgr, r1["bgr"])
        a.close()
        b.close()


def test_context_destroyed_before_its_accumulator():
    """The documented order: rt_ctx_destroy frees the sums of the accumulators still alive; afterwards
    rt_accum_destroy is the only valid call, and every other answers RT_E_INVALID."""
    spec = scenes.config3(96, 64, n=300)
    ctx = lr.Context(0)
    ctx.upload(lr.Scene.deserialize(spec.to_text()))
    acc = ctx.accumulator(opts(spec, 7))
    acc.add(2, PATH)
    ctx.close()
    n = ctypes.c_uint32()
    assert lr.lib.rt_accum_samples(acc._h, ctypes.byref(n)) == lr.RT_OK and n.value == 2
    assert lr.lib.rt_accum_reset(acc._h) == lr.RT_E_INVALID
    acc.close()
    acc.close()                                              # idempotent in the binding


# ---- CLI ----

def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=100)


def test_cli_progressive_and_checkpoint(tmp_path):
    spec = scenes.config3(32, 24, n=100)
    spec.antialias = 5
    scene = str(tmp_path / "scene.txt")
    with open(scene, "w") as f:
        f.write(spec.to_text())
    common = ["--scene", scene, "--algo", "wavefront-aa", "--jitter", "random", "--seed", "77", "--max-depth", spec.max_depth]
    plain, prog, ck1, ck2 = (str(tmp_path / n) for n in ("plain.bmp", "prog.bmp", "ck1.bmp", "ck2.bmp"))
    r = _cli(*common, "--spp", 5, "--out", plain)
    assert r.returncode == 0, r.stdout + r.stderr
    r = _cli(*common, "--spp", 5, "--out", prog, "--progressive", 2)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.findall(r"samples (\d+)/5", r.stderr) == ["2", "4", "5"], r.stderr
    assert open(prog, "rb").read() == open(plain, "rb").read()
    assert not os.path.exists(prog + ".tmp")
    # stop after the first step (--spp 2), then continue to 5 from the checkpoint
    ck = str(tmp_path / "render.ckpt")
    r = _cli(*common, "--spp", 2, "--out", ck1, "--progressive", 2, "--checkpoint", ck)
    assert r.returncode == 0 and os.path.exists(ck), r.stdout + r.stderr
    assert lr.checkpoint_read(ck, header_only=True)[1:3] == (lr.scene_hash(spec.to_text()), 2)
    r = _cli(*common, "--spp", 5, "--out", ck2, "--progressive", 2, "--checkpoint", ck)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "resum" in r.stderr and re.findall(r"samples (\d+)/5", r.stderr) == ["4", "5"], r.stderr
    assert open(ck2, "rb").read() == open(plain, "rb").read()
    assert open(ck1, "rb").read() != open(plain, "rb").read()
    # a checkpoint of another seed is refused
    r = _cli(*[("78" if a == "77" else a) for a in common], "--spp", 5, "--out", ck2, "--checkpoint", ck)
    assert r.returncode != 0 and "checkpoint" in (r.stdout + r.stderr), r.stdout + r.stderr
    # single-device options
    r = _cli(*common, "--spp", 5, "--out", ck2, "--progressive", 2, "--gpus", 2)
    assert r.returncode != 0 and "--gpus" in (r.stdout + r.stderr)
