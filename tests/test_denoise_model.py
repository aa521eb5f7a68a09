"""The numpy model of the denoiser (tests/denoise_model.py) pinned on the CPU, before any device is compared with it
(test_gpu_denoise.py); no GPU.

* the vectorised model equals a plain scalar-loop restatement of the header's rule bit for bit, on small random
  images that include NaN and inf colours, NaN depths, zero normals, zero albedo channels and -0.0;
* what the header says follows from the rule does: a constant dyadic image is a fixed point under every flag mask,
  an edge between orthogonal normals survives RT_DN_NORMAL untouched, non-finite pixels stay where they were and
  spoil nobody else;
* the bytes are output_model's quantisation of the model's f64 values;
* on two noisy renders of the keyed oracle (4 spp, random jitter) guided by aov_model's buffers, the filter lowers
  the mean squared error against a 512-spp render;
* the planner's refusals and per-pass plan (tests/native/denoise_plan_check.cpp, built with the host sanitizers as a
  stand-alone program), the ABI version and the exported symbols.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libraytrace as lr
from libraytrace import scenes
from oracle import ref64

import aov_model as am
import denoise_model as dm
import output_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-raytrace_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
CXXFLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-O1", "-g", "-I" + CSRC,
            "-I" + os.path.join(ROOT, "include")]
SAN = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def f64_same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("shape,seed,special", [((5, 7), 1, False), ((6, 9), 2, True), ((9, 6), 3, True), ((1, 1), 4, False),
                                                ((3, 1), 5, True)])
def test_model_equals_the_scalar_loops(shape, seed, special):
    h, w = shape
    rgb, nrm, depth, albedo = dm.random_image(h, w, seed, special)
    for flags in dm.ALL_MASKS:
        kw = dict(iterations=3, flags=flags, normal_squarings=2, sigma_color=0.7, sigma_depth=0.3)
        m = dm.denoise(rgb, nrm, depth, albedo, **kw)
        v, f32 = dm.scalar_denoise(rgb, nrm, depth, albedo, **kw)
        assert f64_same(m["v"], v), (shape, flags)
        assert dm.same_f32(m["rgb"], f32), (shape, flags)
    if special and h * w >= 40:                               # the special values did reach the filter
        assert np.isnan(rgb).any() and np.isinf(rgb).any() and np.isnan(depth).any()
        assert (albedo == 0).any() and np.signbit(rgb[rgb == 0]).any() and (nrm == 0).all(axis=2).any()


def test_one_pass_against_the_scalar_loops_at_every_squaring_count():
    rgb, nrm, depth, _ = dm.random_image(7, 8, 11, True)
    for sq in (0, 1, 10):
        for s in (1, 2, 4):
            a, _, _ = dm.filter_pass(rgb, s, 7, nrm, depth, sq, 0.5, 0.2)
            assert f64_same(a, dm.scalar_pass(rgb, s, 7, nrm, depth, sq, 0.5, 0.2)), (sq, s)


@pytest.mark.parametrize("flags", dm.ALL_MASKS)
def test_constant_dyadic_image_is_a_fixed_point(flags):
    h, w = 21, 19
    rgb = np.empty((h, w, 3), np.float32)
    rgb[:] = (0.75, 0.125, 2.5)
    nrm = np.zeros((h, w, 3), np.float32)
    nrm[:] = (0.0, 0.0, 1.0)
    depth = np.full((h, w), 3.5, np.float32)
    albedo = np.empty((h, w, 3), np.float32)
    albedo[:] = (0.5, 0.25, 1.0)
    m = dm.denoise(rgb, nrm, depth, albedo, iterations=5, flags=flags, normal_squarings=5, sigma_color=1.0, sigma_depth=0.05)
    assert dm.same_f32(m["rgb"], rgb)                         # borders included: fewer taps, the same quotient
    assert f64_same(m["v"], rgb.astype(np.float64))


def test_orthogonal_normals_keep_their_edge():
    h, w = 16, 24
    rgb = np.empty((h, w, 3), np.float32)
    rgb[:, :12] = (0.3, 0.6, 0.9)
    rgb[:, 12:] = (1.7, 0.2, 0.05)
    nrm = np.zeros((h, w, 3), np.float32)
    nrm[:, :12] = (1.0, 0.0, 0.0)
    nrm[:, 12:] = (0.0, 1.0, 0.0)
    m = dm.denoise(rgb, nrm, iterations=5, flags=dm.NORMAL, normal_squarings=0)
    assert not dm.same_f32(dm.denoise(rgb, iterations=1, flags=0)["rgb"], rgb)      # a plain blur does cross it
    # within a half every kept weight multiplies the same colour: sum / wsum is that colour up to the roundings of
    # the products and of the quotient, which the f32 rounding between passes absorbs
    assert dm.same_f32(m["rgb"], rgb)
    assert (m["kept"][0][:, 11] < m["kept"][0][:, 2]).all()   # the edge column lost its taps across


def test_non_finite_pixels_stay_where_they_were():
    rgb, nrm, depth, albedo = dm.random_image(18, 23, 21, True)
    bad = ~np.isfinite(rgb)
    for flags in (0, dm.NORMAL | dm.DEPTH, dm.COLOR, 7):
        m = dm.denoise(rgb, nrm, depth, albedo, iterations=4, flags=flags, normal_squarings=1, sigma_color=0.8, sigma_depth=0.4)
        assert np.array_equal(~np.isfinite(m["rgb"]), bad), flags
        assert np.array_equal(np.isnan(m["rgb"]), np.isnan(rgb)) and np.array_equal(m["rgb"][np.isinf(rgb)], rgb[np.isinf(rgb)])
    # a NaN depth keeps the pixel's own colour and its neighbours skip it
    clean = np.where(np.isfinite(rgb), rgb, np.float32(0.5)).astype(np.float32)
    clean = np.where(clean == 0, np.float32(0.0), clean)      # (a -0.0 comes back as +0.0: the sums start from +0.0)
    m = dm.denoise(clean, nrm, depth, iterations=3, flags=dm.DEPTH, sigma_depth=0.4)
    assert np.isnan(depth).any() and dm.same_f32(m["rgb"][np.isnan(depth)], clean[np.isnan(depth)])
    assert (m["kept"][0][np.isnan(depth)] == 1).all()


def test_bytes_are_the_output_models():
    rgb, nrm, depth, albedo = dm.random_image(12, 10, 31, True)
    m = dm.denoise(rgb, nrm, depth, albedo, iterations=2, flags=15, normal_squarings=1, bgr_pitch=36)
    assert m["bgr"].shape == (12, 36) and not m["bgr"][:, 30:].any()
    assert np.array_equal(m["bgr"][:, :30].reshape(12, 10, 3)[:, :, ::-1], om.quantise(m["v"]))
    assert np.array_equal(om.quantise(m["v"]), om.binary_search(m["v"]).reshape(12, 10, 3))
    assert dm.same_f32(m["rgb"], om.to_f32(m["v"]))
    assert (om.quantise(m["v"])[np.isnan(m["v"])] == 255).all()


def _mse(a, b):
    d = np.clip(a.astype(np.float64), 0.0, 1.0) - np.clip(b.astype(np.float64), 0.0, 1.0)
    return float((d * d).mean())


@pytest.mark.parametrize("name", ["config1", "stochastic"])
def test_denoised_render_is_closer_to_the_converged_one(name):
    """Keyed oracle, random jitter, 4 spp, guided by aov_model's normal and depth: 5 iterations, NORMAL | DEPTH,
    normal_squarings 5, sigma_depth 0.05.  The prototype measured 0.1188 -> 0.0344 (config1) and 3.13e-4 -> 7.85e-5
    (stochastic) against the 512-spp render."""
    spec = scenes.config1(64, 64, antialias=4, max_depth=2) if name == "config1" else scenes.stochastic(96, 64)
    seed = 7
    noisy = ref64.render(spec, jitter=am.RANDOM, rng=1, seed=seed)["rgb64"].astype(np.float32)
    ref_spec = scenes.config1(64, 64, antialias=512, max_depth=2) if name == "config1" else scenes.stochastic(96, 64, antialias=512)
    converged = ref64.render(ref_spec, jitter=am.RANDOM, rng=1, seed=seed)["rgb64"].astype(np.float32)
    g = am.aov(spec, 4, am.RANDOM, seed)
    m = dm.denoise(noisy, g["normal"], g["depth"], **dm.DEFAULTS)
    before, after = _mse(noisy, converged), _mse(m["rgb"], converged)
    print(f"{name}: noisy MSE {before:.6g}, denoised MSE {after:.6g}")
    assert after < before


def test_denoise_planner(tmp_path):
    exe = str(tmp_path / "denoise_plan_check")
    cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + SAN + ["-o", exe, os.path.join(NATIVE, "denoise_plan_check.cpp"),
                                                            os.path.join(CSRC, "render_plan.cpp")]
    cc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout
    assert "denoise_plan_check ok" in run.stdout


def test_entry_points_are_declared_and_exported():
    names = lr.header_functions()
    assert "rt_denoise" in names and "rt_denoise_device" in names
    assert hasattr(lr.lib, "rt_denoise") and hasattr(lr.lib, "rt_denoise_device")
    assert lr.RT_ABI_VERSION == 10 == lr.lib.rt_abi_version()
    assert (lr.RT_DN_NORMAL, lr.RT_DN_DEPTH, lr.RT_DN_COLOR, lr.RT_DN_DEMODULATE) == (1, 2, 4, 8)
    assert (dm.NORMAL, dm.DEPTH, dm.COLOR, dm.DEMODULATE) == (1, 2, 4, 8)
    assert C.sizeof(lr.rt_denoise_params) == 48 and C.sizeof(lr.rt_denoise_inputs) == 4 * C.sizeof(C.c_void_p)
    assert lr.rt_denoise_params.sigma_color.offset == 32 and lr.rt_denoise_params.sigma_depth.offset == 40
    assert "aa_wavefront" == lr.tuning_keys()[-1]             # no new tuning key
    # a null context is refused before anything is touched
    p, i = lr.denoise_params(8, 8), lr.rt_denoise_inputs()
    assert lr.lib.rt_denoise(None, C.byref(p), C.byref(i), None, None) == lr.RT_E_INVALID
    assert lr.lib.rt_denoise_device(None, C.byref(p), C.byref(i), None, None, None) == lr.RT_E_INVALID
