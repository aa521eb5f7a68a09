"""Moments accumulators on the device (include/raytrace_amd.h, "second moments").

The oracle never returns a single sample's colour, so the tests obtain every sample another way, through the
parent's code path: a PLAIN accumulator, upload(zeros, k), add(1), download() gives 0.0 + s_k.  The stack of
those colours is checked against the oracle through the model (its in-order sum is the oracle's spp = n image
times n) and is the same on the path kernel and on the passes.  Everything else compares the device's sums of
squares with tests/moments_model.py's accumulate of that stack, and noise() with its estimate, bit for bit (f32
outputs as bits; a NaN equals any NaN, IEEE leaving its payload open).  For every split that could show it, the
test also asserts that the other order (a call's squares summed among themselves first) gives other bits on the
very stack it compares with.  Scenes, seeds and helpers are test_gpu_progressive.py's, imported.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import libraytrace as lr
from libraytrace import scenes
import adversarial_scenes
import moments_model as model
import test_gpu_progressive as tgp
from test_gpu_progressive import AA, AUTO, PATH, add, bits, opts, oracle, tuning

pytestmark = pytest.mark.gpu

MOMENTS_LINE = re.compile(r"rtamd: accumulate samples \[\d+, \d+\) (?:path|passes) moments\n")
TILE = dict(x0=24, tile_w=48, y0=16, tile_h=32)          # of test_gpu_progressive's 96 x 64 config3 frame
FLOOR, THRESHOLD = 1e-3, 0.05


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((u64(a) == u64(b)) | (np.isnan(a) & np.isnan(b))).all())


def same32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def upload(ctx, spec, **tune):
    with tuning(ctx, **tune):
        ctx.upload(lr.Scene.deserialize(spec.to_text()))


_stacks = {}


def sample_stack(ctx, key, spec, seed, n, algo=PATH, **okw):
    """[n, h, w, 3]: 0.0 + s_k for k in [0, n), each from a plain accumulator (the scene must be uploaded).
    Computed once per key and left unchanged."""
    k = (key, seed, n, algo, tuple(sorted(okw.items())))
    if k not in _stacks:
        out = []
        with ctx.accumulator(opts(spec, seed, **okw)) as acc:
            assert not acc.has_moments
            zeros = np.zeros((acc.tile_h, acc.tile_w, 3))
            for i in range(n):
                acc.upload(zeros, i)
                acc.add(1, algo)
                s, cnt = acc.download()
                assert cnt == i + 1
                out.append(s)
        _stacks[k] = np.stack(out)
        _stacks[k].setflags(write=False)
    return _stacks[k]


def run_split(ctx, capfd, spec, seed, split, algos, moments, **okw):
    """A fresh accumulator, the split's calls -> (S, Q or None, [(rays, shadow rays) per call], accumulator)."""
    acc = ctx.accumulator(opts(spec, seed, **okw), moments=moments)
    assert acc.has_moments == moments
    counts = []
    for n, algo in zip(split, algos):
        st, err = add(ctx, capfd, acc, n, algo)
        assert bool(MOMENTS_LINE.search(err)) == moments, err
        counts.append((st.rays, st.shadow_rays))
    S, n = acc.download()
    assert n == sum(split)
    return S, (acc.download_moments() if moments else None), counts, acc


def check_split(ctx, capfd, spec, seed, stack, split, algos, **okw):
    """Plain and moments accumulators over the same calls: S equal bits, Q the model's, rays the plain call's."""
    Sp, _, cp, ap = run_split(ctx, capfd, spec, seed, split, algos, False, **okw)
    ap.close()
    Sm, Q, cm, am = run_split(ctx, capfd, spec, seed, split, algos, True, **okw)
    n = sum(split)
    Smod, Qmod = model.accumulate(stack[:n])
    assert same64(Sm, Sp), "a moments accumulator's sums are not the plain accumulator's"
    assert same64(Sp, Smod)
    bad = ~((u64(Q) == u64(Qmod)) | (np.isnan(Q) & np.isnan(Qmod)))
    assert not bad.any(), f"{bad.sum()} of {Q.size} sums of squares differ from the rule"
    assert cm == cp
    return Sm, Q, am


# ---- the per-sample colours ----

def c3():
    return scenes.config3(96, 64, n=300)


def test_sample_stack_is_the_oracles_and_the_same_on_both_schedules(gpu_ctx):
    spec = c3()
    upload(gpu_ctx, spec)
    a = sample_stack(gpu_ctx, "c3", spec, 7, 9, PATH, **TILE)
    b = sample_stack(gpu_ctx, "c3", spec, 7, 9, AA, **TILE)
    assert np.array_equal(u64(a), u64(b))
    assert (a.max(axis=0) != a.min(axis=0)).any()           # random jitter: the samples differ
    # config3's materials have a specular term, and the device's pow is not libm's to the last bit,
    # so against the oracle this stack holds to the suite's tolerance, as test_gpu_progressive.py's renders do ...
    ref = oracle("c3_96", spec, 8, 7, **TILE)["rgb64"] * 8.0
    S = model.accumulate(a[:8])[0]
    print(f"config3: {(u64(S) != u64(ref)).sum()} of {S.size} sums differ from the oracle's bits, "
          f"max relative difference {np.max(np.abs(S - ref) / np.abs(ref)):.3g}")
    assert np.all(np.abs(S - ref) <= tgp.RTOL * np.abs(ref))
    # ... and bit for bit where the suite already demands the oracle's bits: the unlit cancelling scene
    spec = tgp.cancelling_spheres()
    upload(gpu_ctx, spec)
    a = sample_stack(gpu_ctx, "cancel", spec, 19, 9, PATH)
    b = sample_stack(gpu_ctx, "cancel", spec, 19, 9, AA)
    assert np.array_equal(u64(a), u64(b))
    ref = oracle("cancel", spec, 8, 19)["rgb64"]
    nz = ref[ref != 0.0]
    assert (np.abs(nz) > 1e-300).all()                      # times 8 undoes the division by 8 exactly
    assert np.array_equal(u64(model.accumulate(a[:8])[0]), u64(ref * 8.0))


# ---- splits ----

SPLITS = [(9,), (1, 8), (4, 5), (1, 1, 7), (2, 3, 4)]
SCHEDULES = ["path_g1", "path_g2", "path_g8", "path_g64", "passes_compose0", "passes_compose1", "alternating"]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "+".join(map(str, s)))
def test_splits_follow_sample_order(gpu_ctx, capfd, split, schedule):
    spec = c3()
    upload(gpu_ctx, spec)
    stack = sample_stack(gpu_ctx, "c3", spec, 7, 9, PATH, **TILE)
    if len(split) > 1:                                      # this stack tells the orders apart
        Q = model.accumulate(stack)[1]
        assert (u64(model.squares_first(stack, split)) != u64(Q)).sum() >= Q.size // 100
    if schedule.startswith("path"):
        G = int(schedule[6:])
        tune, algos = dict(path_group=G), [PATH] * len(split)
    elif schedule.startswith("passes"):
        tune, algos = dict(compose=int(schedule[-1])), [AA] * len(split)
    else:
        tune, algos = {}, [(PATH, AA)[i % 2] for i in range(len(split))] if len(split) > 1 else [AA]
    with tuning(gpu_ctx, **tune):
        _, _, acc = check_split(gpu_ctx, capfd, spec, 7, stack, split, algos, **TILE)
    acc.close()


def test_second_trip_of_the_persistent_loop_with_groups(gpu_ctx, capfd):
    """test_gpu_progressive's tuning: 64 x 48 pixels x 64 lanes are more work-items than the persistent grid
    has, so every group takes a second pixel, loading and storing that pixel's six doubles."""
    spec = scenes.config2(64, 48)
    upload(gpu_ctx, spec)
    stack = sample_stack(gpu_ctx, "c2_64", spec, 17, 5, PATH)
    with tuning(gpu_ctx, path_group=64):
        acc = gpu_ctx.accumulator(opts(spec, 17), moments=True)
        for n in (2, 3):
            _, err = add(gpu_ctx, capfd, acc, n, PATH)
            m = tgp.PATH_LINE.search(err)
            assert int(m.group(1)) == 64 and int(m.group(4)) * 64 > int(m.group(2)), err
    S, Q = model.accumulate(stack)
    assert same64(acc.download()[0], S) and same64(acc.download_moments(), Q)
    acc.close()


# ---- geometry ----

def test_chunked_passes_address_the_squares_by_row(gpu_ctx, capfd):
    spec = scenes.config3(128, 96)
    upload(gpu_ctx, spec)
    stack = sample_stack(gpu_ctx, "c3_128", spec, 31, 3, PATH)
    for tune in (dict(chunk_pixels=128 * 32), dict(chunk_pixels=128 * 32, lanes=2, compose=1)):
        with tuning(gpu_ctx, **tune):
            acc = gpu_ctx.accumulator(opts(spec, 31), moments=True)
            for n in (1, 2):
                st, _ = add(gpu_ctx, capfd, acc, n, AA)
                assert st.chunks == 3
        S, Q = model.accumulate(stack)
        assert same64(acc.download()[0], S) and same64(acc.download_moments(), Q)
        acc.close()


@pytest.mark.parametrize("algo", [PATH, AA])
def test_tile_offsets_bands_and_pitch(gpu_ctx, capfd, algo):
    spec = c3()
    upload(gpu_ctx, spec)
    tile = dict(x0=5, tile_w=17, y0=3, tile_h=13)
    stack = sample_stack(gpu_ctx, "c3", spec, 7, 3, PATH, **tile)
    _, _, acc = check_split(gpu_ctx, capfd, spec, 7, stack, (1, 2), [algo] * 2, **tile)
    with gpu_ctx.accumulator(opts(spec, 7, **tile)) as plain:
        plain.add(3, algo)
        for pitch in (3 * 17 + 5, 3 * 17 + 2):             # a padded bgr_pitch: the resolve is the plain one's
            a, b = acc.resolve(pitch=pitch), plain.resolve(pitch=pitch)
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    acc.close()
    bands = dict(tile_h=24, band=4, band_stride=2, band_phase=1)
    stack = sample_stack(gpu_ctx, "c3", spec, 7, 3, PATH, **bands)
    _, _, acc = check_split(gpu_ctx, capfd, spec, 7, stack, (2, 1), [algo] * 2, **bands)
    acc.close()


def test_path_only_classes_and_a_tree_beyond_lds(gpu_ctx, capfd):
    spec = scenes.stochastic(48, 32, antialias=3, samples=1)
    spec.objects = [o for o in spec.objects if o["material"]["kind"] != "indirect_phong"]
    spec.plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), scenes.phong((0.6, 0.6, 0.6), (0.2, 0.2, 0.2), 16.0, (0.01,) * 3))
    upload(gpu_ctx, spec)
    stack = sample_stack(gpu_ctx, "stoch", spec, 5, 4, PATH)
    _, _, acc = check_split(gpu_ctx, capfd, spec, 5, stack, (1, 3), [PATH, AUTO])
    with pytest.raises(lr.RtError) as e:
        acc.add(1, AA)
    assert e.value.code == lr.RT_E_UNSUPPORTED and acc.samples == 4
    acc.close()
    # config4: the tree does not fit LDS, the path kernel reads it through the caches (kNodes = 0)
    spec = scenes.config4(64, 48)
    tile = dict(x0=8, tile_w=24, y0=16, tile_h=16)
    upload(gpu_ctx, spec)
    stack = sample_stack(gpu_ctx, "c4", spec, 5, 3, AA, **tile)
    _, _, acc = check_split(gpu_ctx, capfd, spec, 5, stack, (1, 2), [PATH, PATH], **tile)
    acc.close()
    acc = gpu_ctx.accumulator(opts(spec, 5, **tile), moments=True)
    _, err = add(gpu_ctx, capfd, acc, 2, PATH)
    assert tgp.PATH_LINE.search(err).group(3) == "0", err   # staged 0
    _, _, acc2 = check_split(gpu_ctx, capfd, spec, 5, stack, (1, 2), [AA, AA], **tile)
    acc.close()
    acc2.close()


# ---- huge, negative zero, NaN ----

@pytest.mark.parametrize("schedule", ["path_g1", "path_g8", "passes_compose0", "passes_compose1"])
def test_cancelling_scene_across_the_call_boundary(gpu_ctx, capfd, schedule):
    """Ambient +-2^100: S cancels to order 1, Q does not: about 2^200 n."""
    spec = tgp.cancelling_spheres()
    upload(gpu_ctx, spec)
    stack = sample_stack(gpu_ctx, "cancel", spec, 19, 9, PATH)[:5]
    tune = dict(path_group=int(schedule[6:])) if schedule.startswith("path") else dict(compose=int(schedule[-1]))
    algo = PATH if schedule.startswith("path") else AA
    for split in ((2, 3), (1, 4)):
        with tuning(gpu_ctx, **tune):
            _, Q, acc = check_split(gpu_ctx, capfd, spec, 19, stack, split, [algo] * 2)
        assert (Q >= 2.0 ** 198).any() and np.isfinite(Q).all()
        est = model.estimate(*model.accumulate(stack), 5, FLOOR, THRESHOLD)
        var, err, above = acc.noise(FLOOR, THRESHOLD)
        assert same32(var, est["variance"]) and same32(err, est["error"]) and above == est["above"]
        assert np.isinf(var).any()                          # 2^200 does not fit f32: (float)v is inf
        acc.close()


@pytest.mark.parametrize("algo", [PATH, AA])
def test_negative_zero_nan_and_a_reset_over_nan(gpu_ctx, capfd, algo):
    spec = adversarial_scenes.tiny(width=24, height=16)
    spec.background = (-0.0, 0.0, -0.0)
    spec.sphere((0.0, 0.0, -4.0), 1.0, scenes.phong((0.0,) * 3, (0.0,) * 3, 1.0, (0.5, 0.25, -0.0)))
    nan = adversarial_scenes.tiny(width=24, height=16)
    nan.background = (-0.0, 0.0, -0.0)
    nan.sphere((0.0, 0.0, -4.0), 1.0, scenes.phong((0.0,) * 3, (0.0,) * 3, 1.0, (0.5, 0.25, -0.0)))
    nan.plane((0, 0, 0), (0, 0, 0), scenes.phong((0.1, 0.2, 0.3), (0.2, 0.2, 0.2), 4.0, (0, 0, 1)))
    nan.point_light((3, 3, 3), (1, 1, 1))
    upload(gpu_ctx, spec)
    stack = sample_stack(gpu_ctx, "neg_zero", spec, 29, 3, PATH)
    S, Q, acc = check_split(gpu_ctx, capfd, spec, 29, stack, (1, 2), [algo] * 2)
    assert not np.signbit(S).any() and not np.signbit(Q).any() and (Q == 0.0).any()
    # the NaN scene: every sum and every square NaN, every pixel above
    upload(gpu_ctx, nan)
    acc.reset()
    add(gpu_ctx, capfd, acc, 1, algo)
    add(gpu_ctx, capfd, acc, 2, algo)
    assert np.isnan(acc.download()[0]).all() and np.isnan(acc.download_moments()).all()
    var, err, above = acc.noise(FLOOR, THRESHOLD)
    assert np.isnan(var).all() and np.isnan(err).all() and above == 24 * 16
    # a reset over NaN, then fresh samples: sample 0 stores without reading, so no stale square survives
    upload(gpu_ctx, spec)
    acc.reset()
    assert (acc.download_moments() == 0.0).all()            # no samples: BLACK, as the sums
    add(gpu_ctx, capfd, acc, 1, algo)
    add(gpu_ctx, capfd, acc, 2, algo)
    Sm, Qm = model.accumulate(stack)
    assert same64(acc.download()[0], Sm) and same64(acc.download_moments(), Qm) and not np.isnan(Qm).any()
    acc.close()


# ---- noise ----

def _hip_buffer(hip, nbytes, fill):
    d = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d), nbytes) == 0
    h = np.full(nbytes, fill, np.uint8)
    assert hip.hipMemcpy(d, h.ctypes.data, nbytes, 1) == 0
    return d


def _hip_read(hip, d, nbytes, dtype):
    h = np.zeros(nbytes, np.uint8)
    assert hip.hipMemcpy(h.ctypes.data, d, nbytes, 2) == 0
    return h.view(dtype)


def synthetic_moments(w, h, n, seed):
    """Sums and squares of a synthetic stack, with the estimate's special cases planted where they fit."""
    rng = np.random.default_rng(seed)
    stack = rng.uniform(0.0, 1.0, (n, h, w, 3)) * rng.uniform(0.0, 2.0, (1, h, w, 1))
    S, Q = model.accumulate(stack)
    S, Q = S.copy(), Q.copy()
    flat_s, flat_q = S.reshape(-1, 3), Q.reshape(-1, 3)
    npix = w * h
    flat_s[0 % npix] = 2.1                                    # constant pixel: d clamps or is tiny
    flat_q[0 % npix] = np.nextafter(2.1 * (2.1 / n), -np.inf)
    if npix > 2:
        flat_s[npix // 2], flat_q[npix // 2] = np.inf, np.inf  # d NaN: above
        flat_s[npix - 1, 1] = np.nan
    return S, Q


@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("w", [1, 63, 64, 65, 130])
def test_noise_against_the_model(gpu_ctx, w, h):
    spec = scenes.config3(160, 16, n=50)                    # a frame wide enough for the 130-pixel tile
    upload(gpu_ctx, spec)
    n = 6
    S, Q = synthetic_moments(w, h, n, 100 * w + h)
    hip = tgp._hip()
    with gpu_ctx.accumulator(opts(spec, 7, x0=3, tile_w=w, y0=2, tile_h=h), moments=True) as acc:
        acc.upload_moments(S, Q, n)
        assert acc.samples == n
        errs = model.estimate(S, Q, n, FLOOR, 1.0)["err"]
        finite = errs[np.isfinite(errs) & (errs > 0.0)]
        pick = float(np.sort(finite)[len(finite) // 2]) if len(finite) else 0.5
        lo, hi = float(np.nextafter(0.0, 1.0)), 1e300
        for thr in (lo, hi, pick, float(np.nextafter(pick, 0.0))):
            est = model.estimate(S, Q, n, FLOOR, thr)
            var, err, above = acc.noise(FLOOR, thr)
            assert same32(var, est["variance"]) and same32(err, est["error"])
            assert above == est["above"], (thr, above, est["above"])
            assert acc.noise(FLOOR, thr, variance=False)[::2] == (None, above)
            assert same32(acc.noise(FLOOR, thr, variance=False)[1], est["error"])
            assert same32(acc.noise(FLOOR, thr, error=False)[0], est["variance"])
            assert acc.noise(FLOOR, thr, variance=False, error=False) == (None, None, above)   # the count alone
            assert acc.noise_device(FLOOR, thr) == above                                        # ... and again: cleared per call
        # thresholds below every finite err, above every err, at one pixel's exact err and one step below it
        n_nan = int(np.isnan(errs).sum())
        assert acc.noise_device(FLOOR, hi) == n_nan
        assert acc.noise_device(FLOOR, lo) == int((~(errs <= lo)).sum())
        if len(finite):
            at, below = acc.noise_device(FLOOR, pick), acc.noise_device(FLOOR, float(np.nextafter(pick, 0.0)))
            assert below - at == int((errs == pick).sum()) >= 1
        # device buffers with guards around them
        est = model.estimate(S, Q, n, FLOOR, THRESHOLD)
        guard, nv, ne = 256, w * h * 12, w * h * 4
        d_var, d_err = _hip_buffer(hip, guard + nv + guard, 0xCD), _hip_buffer(hip, guard + ne + guard, 0xCD)
        try:
            above = acc.noise_device(FLOOR, THRESHOLD, d_var.value + guard, d_err.value + guard)
            hv = _hip_read(hip, d_var, guard + nv + guard, np.uint8)
            he = _hip_read(hip, d_err, guard + ne + guard, np.uint8)
        finally:
            hip.hipFree(d_var)
            hip.hipFree(d_err)
        assert above == est["above"]
        assert (hv[:guard] == 0xCD).all() and (hv[guard + nv:] == 0xCD).all(), "guard bytes written"
        assert (he[:guard] == 0xCD).all() and (he[guard + ne:] == 0xCD).all(), "guard bytes written"
        assert same32(hv[guard:guard + nv].view(np.float32).reshape(h, w, 3), est["variance"])
        assert same32(he[guard:guard + ne].view(np.float32).reshape(h, w), est["error"])
        # S and Q are read, never written
        assert np.array_equal(u64(acc.download()[0]), u64(S)) and np.array_equal(u64(acc.download_moments()), u64(Q))


def test_noise_of_a_render_and_its_ordering(gpu_ctx, capfd):
    """noise() right after an asynchronous accumulate, and an accumulate right after a device noise call."""
    spec = c3()
    upload(gpu_ctx, spec)
    stack = sample_stack(gpu_ctx, "c3", spec, 7, 9, PATH, **TILE)
    with gpu_ctx.accumulator(opts(spec, 7, **TILE), moments=True) as acc:
        acc.add(4, AA)
        above4 = acc.noise_device(FLOOR, THRESHOLD)
        acc.add(5, PATH)
        var, err, above9 = acc.noise(FLOOR, THRESHOLD)
        e4 = model.estimate(*model.accumulate(stack[:4]), 4, FLOOR, THRESHOLD)
        e9 = model.estimate(*model.accumulate(stack), 9, FLOOR, THRESHOLD)
        assert (above4, above9) == (e4["above"], e9["above"])
        assert same32(var, e9["variance"]) and same32(err, e9["error"])
        assert 0 < e9["above"] < 48 * 32                    # the threshold separates this scene's pixels
        # timed as compose when the last accumulate was timed
        gpu_ctx.kernel_times()
        acc.noise(FLOOR, THRESHOLD)
        assert gpu_ctx.kernel_times()["compose"][1] == 0
        add(gpu_ctx, capfd, acc, 1, PATH, flags=lr.RT_TIME_KERNELS)
        gpu_ctx.kernel_times()
        acc.noise(FLOOR, THRESHOLD)
        assert gpu_ctx.kernel_times()["compose"][1] == 1


# ---- lifecycle ----

@pytest.mark.parametrize("through_file", [False, True])
def test_download_upload_continues_in_a_fresh_context(gpu_ctx, capfd, tmp_path, through_file):
    spec = c3()
    text = spec.to_text()
    upload(gpu_ctx, spec)
    stack = sample_stack(gpu_ctx, "c3", spec, 7, 9, PATH, **TILE)
    o = opts(spec, 7, **TILE)
    with gpu_ctx.accumulator(o, moments=True) as acc:
        add(gpu_ctx, capfd, acc, 4, AA)
        S, n = acc.download()
        Q = acc.download_moments()
    if through_file:
        path = str(tmp_path / "render.ckpt")
        lr.checkpoint_write_moments(path, o, lr.scene_hash(text), n, S, Q)
        o2, h, n2, S2, Q2 = lr.checkpoint_read_moments(path)
        assert (h, n2, o2.tile_w, o2.x0) == (lr.scene_hash(text), 4, 48, 24)
        assert np.array_equal(u64(S2), u64(S)) and np.array_equal(u64(Q2), u64(Q))
        with pytest.raises(lr.RtError) as e:
            lr.checkpoint_read(path)                        # the version 1 reader still refuses version 2
        assert e.value.code == lr.RT_E_INVALID
        S, Q, n = S2, Q2, n2
    with lr.Context(0) as ctx:
        ctx.upload(lr.Scene.deserialize(text))
        with ctx.accumulator(o, moments=True) as acc:
            acc.upload_moments(S, Q, n)
            assert acc.samples == 4
            add(ctx, capfd, acc, 5, PATH)
            Sm, Qm = model.accumulate(stack)
            assert same64(acc.download()[0], Sm) and same64(acc.download_moments(), Qm)


def test_reserved_accumulate_allocates_nothing(capfd):
    spec = c3()
    with lr.Context(0, tuning={"verbose": 1}) as ctx:
        ctx.upload(lr.Scene.deserialize(spec.to_text()))
        ctx.reserve(opts(spec, 7, spp=3, algo=AA, **TILE))
        assert tgp.GROWN.search(capfd.readouterr().err)
        with ctx.accumulator(opts(spec, 7, **TILE), moments=True) as acc:
            capfd.readouterr()
            acc.add(3, AA)
            ctx.stats()
            err = capfd.readouterr().err
            assert MOMENTS_LINE.search(err) and not tgp.GROWN.search(err) and "released" not in err, err
            assert acc.noise(FLOOR, THRESHOLD)[2] >= 0


def test_context_destroyed_before_its_accumulator():
    spec = c3()
    ctx = lr.Context(0)
    ctx.upload(lr.Scene.deserialize(spec.to_text()))
    acc = ctx.accumulator(opts(spec, 7, **TILE), moments=True)
    acc.add(2, PATH)
    ctx.close()
    n, f = ctypes.c_uint32(), ctypes.c_int32()
    assert lr.lib.rt_accum_samples(acc._h, ctypes.byref(n)) == lr.RT_OK and n.value == 2
    assert lr.lib.rt_accum_has_moments(acc._h, ctypes.byref(f)) == lr.RT_OK and f.value == 1
    assert lr.lib.rt_accum_reset(acc._h) == lr.RT_E_INVALID
    acc.close()
    acc.close()


# ---- refusals ----

def test_refusals_change_nothing(gpu_ctx, capfd):
    spec = c3()
    upload(gpu_ctx, spec)
    npx = 48 * 32 * 3
    plain = gpu_ctx.accumulator(opts(spec, 7, **TILE))
    acc = gpu_ctx.accumulator(opts(spec, 7, **TILE), moments=True)
    add(gpu_ctx, capfd, plain, 2, PATH)
    add(gpu_ctx, capfd, acc, 1, PATH)
    st0 = gpu_ctx.stats()

    def state(a):
        return (a.samples, u64(a.download()[0]).copy(), u64(a.download_moments()).copy() if a.has_moments else None)

    def refused(a, fn, text=None):
        before = state(a)
        with pytest.raises(lr.RtError) as e:
            fn()
        assert e.value.code == lr.RT_E_INVALID, str(e.value)
        assert text is None or text in str(e.value), str(e.value)
        after, st = state(a), gpu_ctx.stats()
        assert before[0] == after[0] and np.array_equal(before[1], after[1])
        assert before[2] is None or np.array_equal(before[2], after[2])
        assert (st.rays, st.shadow_rays, st.pixels) == (st0.rays, st0.shadow_rays, st0.pixels)

    # a plain accumulator has no squares
    refused(plain, lambda: plain.noise(FLOOR, THRESHOLD), "rt_accum_create_moments")
    refused(plain, lambda: plain.noise_device(FLOOR, THRESHOLD))
    refused(plain, plain.download_moments)
    refused(plain, lambda: plain.upload_moments(np.zeros(npx), np.zeros(npx), 2))
    # a moments accumulator's sums cannot be replaced alone
    refused(acc, lambda: acc.upload(np.zeros(npx), 1), "stale")
    refused(acc, lambda: acc.upload_moments(np.zeros(npx - 3), np.zeros(npx - 3), 1))
    refused(acc, lambda: acc.upload_moments(np.zeros(npx), np.zeros(npx), 2 ** 31 + 1))
    refused(acc, lambda: acc.download_moments(cap=npx - 1))
    # one sample is no variance
    refused(acc, lambda: acc.noise(FLOOR, THRESHOLD), "2 samples")
    refused(acc, lambda: acc.noise_device(FLOOR, THRESHOLD), "2 samples")
    add(gpu_ctx, capfd, acc, 1, PATH)
    st0 = gpu_ctx.stats()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(acc, lambda: acc.noise(bad, THRESHOLD), "floor")
        refused(acc, lambda: acc.noise(FLOOR, bad), "threshold")
        refused(acc, lambda: acc.noise_device(bad, THRESHOLD), "floor")
        refused(acc, lambda: acc.noise_device(FLOOR, bad), "threshold")
    # *above is left alone by a refused call
    above = ctypes.c_uint64(12345)
    assert lr.lib.rt_accum_noise_host(gpu_ctx._h, acc._h, 0.0, THRESHOLD, None, None, ctypes.byref(above)) == lr.RT_E_INVALID
    assert lr.lib.rt_accum_noise(gpu_ctx._h, plain._h, FLOOR, THRESHOLD, None, None, ctypes.byref(above), None) == lr.RT_E_INVALID
    assert above.value == 12345
    assert acc.noise(FLOOR, THRESHOLD)[2] >= 0              # ... and the accepted call works
    # a stale scene binding
    spec2 = scenes.config2(96, 64)
    spec2.max_depth = spec.max_depth
    upload(gpu_ctx, spec2)
    for fn in (lambda: acc.noise(FLOOR, THRESHOLD), lambda: acc.noise_device(FLOOR, THRESHOLD), acc.download_moments,
               lambda: acc.upload_moments(np.zeros(npx), np.zeros(npx), 2)):
        with pytest.raises(lr.RtError) as e:
            fn()
        assert e.value.code == lr.RT_E_INVALID and "rt_accum_reset" in str(e.value)
    assert acc.samples == 2
    plain.close()
    acc.close()


# ---- CLI ----

def _cli(*args):
    return subprocess.run([tgp.EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=100)


def _read_pfm(path):
    raw = open(path, "rb").read()
    kind, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert kind == b"PF" and float(scale) < 0.0                # 3 channels, little-endian
    return np.frombuffer(body, "<f4").reshape(h, w, 3)


def test_cli_until_noise_variance_and_checkpoint_kind(gpu_ctx, tmp_path):
    spec = scenes.config3(32, 24, n=100)
    spec.antialias = 32
    text = spec.to_text()
    scene = str(tmp_path / "scene.txt")
    with open(scene, "w") as f:
        f.write(text)
    K, spp = 4, 32
    # the same steps through the library: the sums after every step, and the model's estimate of each.  The
    # threshold is the median relative error of the first step's noisy pixels: errors shrink like 1 / sqrt(n),
    # so the count falls as samples are added, and the lowest count of a later step is a P that stops there
    upload(gpu_ctx, spec)
    sums, variances = [], []
    with gpu_ctx.accumulator(opts(spec, 77), moments=True) as acc:
        for _ in range(spp // K):
            acc.add(K, PATH)
            sums.append((acc.download()[0], acc.download_moments()))
            variances.append(acc.noise(FLOOR, 1.0)[0])
    err0 = model.estimate(*sums[0], K, FLOOR, 1.0)["err"]
    T = float(np.median(err0[err0 > 0.0]))
    aboves = [model.estimate(S, Q, K * (i + 1), FLOOR, T)["above"] for i, (S, Q) in enumerate(sums)]
    P = min(aboves[1:])
    stop = next(i for i, a in enumerate(aboves) if a <= P)
    assert stop >= 1, aboves                                   # not at the first step
    T = repr(T)                                                # every digit: the CLI parses the same double
    common = ["--scene", scene, "--algo", "path", "--jitter", "random", "--seed", "77", "--max-depth", spec.max_depth,
              "--spp", spp, "--progressive", K]
    out, var, ck = (str(tmp_path / n) for n in ("out.bmp", "var.pfm", "render.ckpt"))
    r = _cli(*common, "--out", out, "--until-noise", T, "--noise-pixels", P, "--variance", var, "--checkpoint", ck)
    assert r.returncode == 0, r.stdout + r.stderr
    final = int(re.search(r"stopped at (\d+) samples", r.stderr).group(1))
    assert final % K == 0 and final == K * (stop + 1), (final, aboves, r.stderr)
    assert [int(a) for a in re.findall(r"noise above (\d+)", r.stderr)] == aboves[:stop + 1]
    assert aboves[stop] <= P < aboves[stop - 1]                # the model: converged there, not a step earlier
    assert re.findall(r"samples (\d+)/32", r.stderr) == [str(K * (i + 1)) for i in range(stop + 1)]
    assert same32(_read_pfm(var), variances[stop])
    # the checkpoint is of the moments kind; a run without moments leaves it alone and starts fresh, and the other way round
    assert lr.checkpoint_read_moments(ck, header_only=True)[1:3] == (lr.scene_hash(text), final)
    with pytest.raises(lr.RtError):
        lr.checkpoint_read(ck, header_only=True)
    r = _cli(*common[:-4], "--spp", K, "--progressive", K, "--out", out, "--checkpoint", ck)
    assert r.returncode == 0 and "starting fresh" in r.stderr and "resuming" not in r.stderr, r.stdout + r.stderr
    assert lr.checkpoint_read(ck, header_only=True)[2] == K
    r = _cli(*common, "--out", out, "--until-noise", T, "--noise-pixels", P, "--checkpoint", ck)
    assert r.returncode == 0 and "starting fresh" in r.stderr, r.stdout + r.stderr
    assert f"stopped at {final} samples" in r.stderr
    # ... and a moments run resumes from its own kind: stop after one step, then continue
    os.remove(ck)
    r = _cli(*common[:-4], "--spp", K, "--progressive", K, "--out", out, "--variance", var, "--checkpoint", ck)
    assert r.returncode == 0, r.stdout + r.stderr
    assert same32(_read_pfm(var), variances[0])
    r = _cli(*common, "--out", out, "--until-noise", T, "--noise-pixels", P, "--variance", var, "--checkpoint", ck)
    assert r.returncode == 0 and "resuming" in r.stderr and f"stopped at {final} samples" in r.stderr, r.stdout + r.stderr
    assert same32(_read_pfm(var), variances[stop])
    # ... and from a checkpoint that has converged: the rule is asked before any more samples are traced
    r = _cli(*common, "--out", out, "--until-noise", T, "--noise-pixels", P, "--variance", var, "--checkpoint", ck)
    assert r.returncode == 0 and "resuming" in r.stderr and f"stopped at {final} samples" in r.stderr, r.stdout + r.stderr
    assert [int(a) for a in re.findall(r"noise above (\d+)", r.stderr)] == [aboves[stop]], r.stderr
    assert lr.checkpoint_read_moments(ck, header_only=True)[2] == final
    assert same32(_read_pfm(var), variances[stop])
    # argument checks
    for bad in (["--until-noise", T], ["--progressive", K, "--until-noise", "-1"], ["--progressive", K, "--until-noise", T, "--noise-floor", 0],
                ["--progressive", K, "--until-noise", T, "--gpus", 2], ["--variance", var, "--spp", 1]):
        r = _cli("--scene", scene, "--out", out, *([] if "--spp" in bad else ["--spp", 8]), *bad)
        assert r.returncode != 0, (bad, r.stdout + r.stderr)
