"""The numpy model of the variance-guided denoiser (tests/denoise_var_model.py) pinned on the CPU, before any device is
compared with it (test_gpu_denoise_var.py); no GPU.

* the vectorised model equals a plain scalar-loop restatement of the header's rule bit for bit (colours and
  variances), on small images with NaN and inf colours, NaN depths, zero normals and albedo channels, and a variance
  image sprinkled with NaN, -1, -0.0, 0, +inf, f32 denormals and 2^100;
* what the header says follows from the rule does: with variance 2^100 everywhere the colours and bytes are
  rt_denoise's under every mask; a constant dyadic image is a fixed point for any variance; non-finite pixels keep to
  themselves; every stored variance lies in [0, +inf]; with variance 0 a tap across a colour step e carries at most
  kw * variance_floor / e;
* on the synthetic image the rule was designed on (edges that no guide sees, a noise-free third) the guided filter
  brings the error below a tenth of the input's, where the plain filter with the same guides raises it;
* on two noisy renders of the keyed oracle, with the variance estimated from the per-sample colours, the guided filter
  lowers the error against a 512-spp render (the plain filter's figure is printed beside it, not compared);
* the planner's refusals (tests/native/denoise_var_plan_check.cpp, built with the host sanitizers as a stand-alone
  program), the ABI version, the exported symbols and the struct's layout, also that of its Rust mirror in
  INTEGRATION.md, whose pointer fields test_integration_binding.py's parser does not read.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import libraytrace as lr
from libraytrace import scenes
from oracle import ref64

import aov_model as am
import denoise_model as dm
import denoise_var_model as dv
import moments_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-raytrace_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
CXXFLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-O1", "-g", "-I" + CSRC,
            "-I" + os.path.join(ROOT, "include")]
SAN = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
BIG = np.float32(2.0 ** 100)


def f64_same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("shape,seed", [((5, 7), 1), ((6, 9), 2), ((9, 6), 3), ((1, 1), 4), ((3, 1), 5)])
def test_model_equals_the_scalar_loops(shape, seed):
    h, w = shape
    rgb, nrm, depth, albedo = dm.random_image(h, w, seed, True)
    var = dv.random_variance(h, w, 50 + seed, True)
    for flags in dv.ALL_MASKS:
        kw = dict(iterations=3, flags=flags, normal_squarings=2, sigma_color=0.7, sigma_depth=0.3, sigma_variance=1.5,
                  variance_floor=2.0 ** -12)
        m = dv.denoise_var(rgb, var, nrm, depth, albedo, **kw)
        v, f32, x, x32 = dv.scalar_denoise_var(rgb, var, nrm, depth, albedo, **kw)
        assert f64_same(m["v"], v), (shape, flags)
        assert dm.same_f32(m["rgb"], f32), (shape, flags)
        assert f64_same(m["x"], x), (shape, flags)
        assert dm.same_f32(m["variance"], x32), (shape, flags)
    if h * w >= 40:                                           # the special values did reach the filter
        assert np.isnan(rgb).any() and np.isinf(rgb).any() and np.isnan(depth).any()
        assert np.isnan(var).any() and (var < 0).any() and np.isinf(var).any() and (var == BIG).any()
        assert np.signbit(var[var == 0]).any() and ((var > 0) & (var < np.float32(2.0 ** -126))).any()


def test_pack_against_the_scalar_loops_and_the_rule():
    rgb, _, _, albedo = dm.random_image(9, 11, 12, True)
    var = dv.random_variance(9, 11, 13, True)
    for flags in (0, dv.DEMODULATE):
        p = dv.pack_variance(var, flags, albedo)
        assert dm.same_f32(p, dv.scalar_pack(var, flags, albedo))
        assert (p >= 0).all() and not np.signbit(p).any()     # NaN, negative values and -0.0 became +0.0
    # one channel NaN, the others ordinary: the pixel's variance is the others' sum
    one = np.array([[[np.nan, 0.25, 0.5]]], np.float32)
    assert dv.pack_variance(one, 0)[0, 0] == np.float32(0.75)
    # demodulation divides by the squared albedo where that is > 0
    a = np.array([[[0.5, 0.0, -1.0]]], np.float32)
    assert dv.pack_variance(np.array([[[0.25, 0.25, 0.25]]], np.float32), dv.DEMODULATE, a)[0, 0] == np.float32(1.5)


@pytest.mark.parametrize("flags", dv.ALL_MASKS)
def test_huge_variance_gives_the_plain_filters_bits(flags):
    """Variance 2^100, colours of ordinary magnitude: e / den < 2^-53, every new divisor is 1.0."""
    for (h, w), seed, iterations in (((18, 23), 21, 5), ((9, 40), 22, 8)):
        rgb, nrm, depth, albedo = dm.random_image(h, w, seed, False)
        var = np.full((h, w, 3), BIG, np.float32)
        kw = dict(iterations=iterations, flags=flags, normal_squarings=2, sigma_color=0.7, sigma_depth=0.3)
        plain = dm.denoise(rgb, nrm, depth, albedo, **kw)
        m = dv.denoise_var(rgb, var, nrm, depth, albedo, **kw, **dv.VAR_DEFAULTS)
        assert f64_same(m["v"], plain["v"]) and dm.same_f32(m["rgb"], plain["rgb"]) and np.array_equal(m["bgr"], plain["bgr"])
        assert all(np.array_equal(a, b) for a, b in zip(m["kept"], plain["kept"]))
        assert np.isfinite(m["variance"]).all() and (m["variance"] > 0).all()


@pytest.mark.parametrize("flags", dv.ALL_MASKS)
def test_constant_dyadic_image_is_a_fixed_point_for_any_variance(flags):
    h, w = 21, 19
    rgb = np.empty((h, w, 3), np.float32)
    rgb[:] = (0.75, 0.125, 2.5)
    nrm = np.zeros((h, w, 3), np.float32)
    nrm[:] = (0.0, 0.0, 1.0)
    depth = np.full((h, w), 3.5, np.float32)
    albedo = np.empty((h, w, 3), np.float32)
    albedo[:] = (0.5, 0.25, 1.0)
    for var in (dv.random_variance(h, w, 31, True), np.zeros((h, w, 3), np.float32), np.full((h, w, 3), np.inf, np.float32)):
        m = dv.denoise_var(rgb, var, nrm, depth, albedo, iterations=5, flags=flags, normal_squarings=5, sigma_color=1.0,
                           sigma_depth=0.05, **dv.VAR_DEFAULTS)
        assert dm.same_f32(m["rgb"], rgb)
        assert f64_same(m["v"], rgb.astype(np.float64))


def test_non_finite_pixels_stay_where_they_were():
    rgb, nrm, depth, albedo = dm.random_image(18, 23, 21, True)
    bad = ~np.isfinite(rgb)
    for var in (dv.random_variance(18, 23, 32, True), dv.random_variance(18, 23, 33, False)):
        for flags in (0, dv.NORMAL | dv.DEPTH, dv.COLOR, 7):
            m = dv.denoise_var(rgb, var, nrm, depth, albedo, iterations=4, flags=flags, normal_squarings=1, sigma_color=0.8,
                               sigma_depth=0.4, **dv.VAR_DEFAULTS)
            assert np.array_equal(~np.isfinite(m["rgb"]), bad), flags
            assert np.array_equal(np.isnan(m["rgb"]), np.isnan(rgb)) and np.array_equal(m["rgb"][np.isinf(rgb)], rgb[np.isinf(rgb)])


@pytest.mark.parametrize("flags", [0, 3, 7, 15])
def test_stored_variances_are_never_nan_or_negative(flags):
    rgb, nrm, depth, albedo = dm.random_image(18, 23, 21, True)
    for seed in (34, 35):
        var = dv.random_variance(18, 23, seed, True)
        for sv, floor in ((2.0, 2.0 ** -20), (1e200, 1e-300), (1e-200, 1e300)):
            m = dv.denoise_var(rgb, var, nrm, depth, albedo, iterations=5, flags=flags, normal_squarings=1, sigma_color=0.8,
                               sigma_depth=0.4, sigma_variance=sv, variance_floor=floor)
            for v in m["variances"] + [m["variance"], m["x"]]:
                assert (v >= 0).all() and not np.signbit(v).any(), (flags, seed, sv)      # (a NaN fails v >= 0)
        assert np.isinf(m["variances"][0]).any()              # +inf is a value a variance may have


def test_zero_variance_keeps_a_colour_step():
    """Variance 0: den is the floor, and a tap across a step of squared size e weighs kw / (1 + e / floor) <= kw * floor /
    e.  In the column left of a vertical step the taps across are the columns dx = 1, 2 (kernel weight 5/16 of the
    whole), the others (11/16) have the pixel's own colour A: |v - A| <= |B - A| * (5/11) * floor / e."""
    h, w, floor = 12, 16, 2.0 ** -20
    A, B = np.array((0.75, 0.5, 0.25)), np.array((0.25, 1.0, 0.75))
    e = float(((A - B) ** 2).sum())
    rgb = np.empty((h, w, 3), np.float32)
    rgb[:, :8], rgb[:, 8:] = A, B
    zero = np.zeros((h, w), np.float32)
    v, x, g, _, kept = dv.filter_pass(rgb, zero, 1, 0, sigma_variance=2.0, variance_floor=floor)
    assert (g == 0).all() and (x == 0).all() and (kept[2:-2, 2:-2] == 25).all()       # cut down, not skipped
    bound = np.abs(B - A) * (5.0 / 11.0) * floor / e
    assert (np.abs(v[:, 7] - A) <= bound * (1 + 1e-12)).all() and (np.abs(v[:, 7] - A) > 0).any()
    plain, _, _ = dm.filter_pass(rgb, 1, 0)
    assert np.allclose(np.abs(plain[2:-2, 7] - A), np.abs(B - A) * 5.0 / 16.0)         # what the step loses without it
    # five passes: the step is where it was, to the same order
    m = dv.denoise_var(rgb, np.zeros((h, w, 3), np.float32), iterations=5, flags=0, sigma_variance=2.0, variance_floor=floor)
    assert np.abs(m["v"] - rgb.astype(np.float64)).max() <= 5 * floor / e


def _mse(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float((d * d).mean())


def test_synthetic_image_guided_beats_noisy_and_plain_does_not():
    """Seed 1, floor 1e-6, 4 samples, 5 passes, NORMAL | DEPTH over one normal and depth.  The design's prototype measured
    noisy 0.0148, plain 0.0198, guided (sigma_variance 2) 6.2e-5 on its image; this restatement (the same layout and
    noise, colours and random stream of its own: denoise_var_model.synthetic) measures noisy 0.01483, plain 0.02300,
    guided 4.57e-4 / 2.33e-4 / 4.96e-4 / 1.21e-3 at sigma_variance 1 / 2 / 4 / 8."""
    im = dv.synthetic(seed=1)
    kw = dict(iterations=5, flags=dm.NORMAL | dm.DEPTH, normal_squarings=5, sigma_depth=0.05)
    noisy = _mse(im["noisy"], im["truth"])
    plain = _mse(dm.denoise(im["noisy"], im["normal"], im["depth"], **kw)["rgb"], im["truth"])
    print(f"synthetic: noisy MSE {noisy:.4g}, plain MSE {plain:.4g}")
    guided = {}
    for sv in (1.0, 2.0, 4.0, 8.0):
        m = dv.denoise_var(im["noisy"], im["variance"], im["normal"], im["depth"], sigma_variance=sv, variance_floor=1e-6, **kw)
        guided[sv] = _mse(m["rgb"], im["truth"])
        print(f"synthetic: guided MSE {guided[sv]:.4g} at sigma_variance {sv:g}")
    assert guided[2.0] < noisy / 10.0
    assert plain > noisy
    # the noise-free third, away from the noisy pixels' 3 x 3 reach (variance 0: den is the floor): a tap whose colour is
    # off by sqrt(e) moves the pixel by at most sqrt(e) / (1 + e / floor) <= sqrt(floor) / 2 of its share of the weights
    m = dv.denoise_var(im["noisy"], im["variance"], im["normal"], im["depth"], sigma_variance=2.0, variance_floor=1e-6, **kw)
    assert np.abs(m["rgb"][:, :28] - im["truth"][:, :28]).max() < 5 * 0.5 * 1e-3


def per_sample_variance(spec_of, n, seed):
    """The variance of the mean of an n-sample keyed render, from the oracle's prefix renders: sample k's colours are
    k * mean_k - (k - 1) * mean_(k-1); then moments_model's rule."""
    means = [ref64.render(spec_of(k), jitter=am.RANDOM, rng=1, seed=seed)["rgb64"] for k in range(1, n + 1)]
    samples = [means[0]] + [k * means[k - 1] - (k - 1) * means[k - 2] for k in range(2, n + 1)]
    S, Q = mm.accumulate(np.stack(samples))
    return means[-1].astype(np.float32), mm.estimate(S, Q, n, 1e-3, 1.0)["variance"]


@pytest.mark.parametrize("name", ["config1", "stochastic"])
def test_guided_render_is_closer_to_the_converged_one(name):
    """The two scenes of test_denoise_model.py, 4 spp, guided by aov_model's normal and depth and by the per-sample
    variance.  Measured: config1 noisy 0.1146, plain 0.03354, guided 0.04259; stochastic noisy
    3.083e-4, plain 7.704e-5, guided 1.043e-4: on these two scenes the plain filter is the closer one.  Only
    "guided < noisy" is required."""
    def spec_of(k):
        return scenes.config1(64, 64, antialias=k, max_depth=2) if name == "config1" else scenes.stochastic(96, 64, antialias=k)
    seed = 7
    noisy, var = per_sample_variance(spec_of, 4, seed)
    converged = ref64.render(spec_of(512), jitter=am.RANDOM, rng=1, seed=seed)["rgb64"].astype(np.float32)
    g = am.aov(spec_of(4), 4, am.RANDOM, seed)
    plain = dm.denoise(noisy, g["normal"], g["depth"], **dm.DEFAULTS)
    guided = dv.denoise_var(noisy, var, g["normal"], g["depth"], **dm.DEFAULTS, **dv.VAR_DEFAULTS)

    def mse(a):
        d = np.clip(a.astype(np.float64), 0.0, 1.0) - np.clip(converged.astype(np.float64), 0.0, 1.0)
        return float((d * d).mean())
    print(f"{name}: noisy MSE {mse(noisy):.4g}, plain MSE {mse(plain['rgb']):.4g}, guided MSE {mse(guided['rgb']):.4g}")
    assert mse(guided["rgb"]) < mse(noisy)


def test_denoise_var_planner(tmp_path):
    exe = str(tmp_path / "denoise_var_plan_check")
    cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + SAN + ["-o", exe, os.path.join(NATIVE, "denoise_var_plan_check.cpp"),
                                                            os.path.join(CSRC, "render_plan.cpp")]
    cc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout
    assert "denoise_var_plan_check ok" in run.stdout


def test_rust_mirror_of_the_struct_matches_the_header(tmp_path):
    """INTEGRATION.md's `RtDenoiseVariance` against `rt_denoise_variance`, pointer fields included.
    tests/test_integration_binding.py reads scalar fields only, so it cannot compare a struct that mixes pointers and
    scalars (the mirror is spelled so that it passes it over); this is that struct's check: every field public, the
    header's names in the header's order, the types that correspond, and Rust's repr(C) offsets and size equal to
    offsetof / sizeof from a C probe of the header."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rust = re.sub(r"//[^\n]*", "", "\n".join(re.findall(r"```rust\n(.*?)```", doc, flags=re.S)))
    found = re.findall(r"#\[repr\(C(?:,\s*align\((\d+)\))?\)\][^{;]*?pub struct RtDenoiseVariance\s*\{(.*?)\}", rust, flags=re.S)
    assert len(found) == 1, found
    align_attr, body = found[0]
    decls = [d.strip() for d in body.split(",") if d.strip()]
    rust_fields = []
    for d in decls:
        m = re.fullmatch(r"pub (\w+)\s*:\s*(\*const \w+|\*mut \w+|\w+)", d)
        assert m, f"not a plain `pub name: type` field: {d!r}"
        rust_fields.append((m.group(1), m.group(2)))
    types = {"*const f32": ("const float*", C.sizeof(C.c_void_p)), "*mut f32": ("float*", C.sizeof(C.c_void_p)), "f64": ("double", 8)}
    header = os.path.join(ROOT, "include", "raytrace_amd.h")
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    m = re.search(r"typedef struct\s*\{([^{}]*)\}\s*rt_denoise_variance\s*;", text)
    assert m
    c_fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if decl:
            dm_ = re.fullmatch(r"((?:const )?\w+ ?\*?) ?(\w+)", decl)
            assert dm_, decl
            c_fields.append((dm_.group(2), dm_.group(1).replace(" *", "*").strip()))
    assert [n for n, _ in rust_fields] == [n for n, _ in c_fields]
    probe = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void) {",
             'printf("%zu\\n", sizeof(rt_denoise_variance));']
    probe += [f'printf("%zu %zu\\n", offsetof(rt_denoise_variance, {n}), sizeof(((rt_denoise_variance*)0)->{n}));' for n, _ in c_fields]
    probe.append("return 0; }")
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(probe))
    subprocess.run([os.environ.get("CC", "gcc"), "-std=c11", "-Wall", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    c_size, c_layout = int(out[0]), [tuple(int(v) for v in line.split()) for line in out[1:1 + len(c_fields)]]
    off, align = 0, int(align_attr or 1)
    for (name, rty), (_, cty), (c_off, c_sz) in zip(rust_fields, c_fields, c_layout):
        assert rty in types, (name, rty)
        want_c, sz = types[rty]
        assert cty == want_c, f"{name}: Rust {rty} but the header says {cty}"
        off = (off + sz - 1) // sz * sz                          # repr(C): aligned to the field's size
        assert (c_off, c_sz) == (off, sz), f"{name}: Rust offset {off}, size {sz} vs C {(c_off, c_sz)}"
        off += sz
        align = max(align, sz)
    assert (off + align - 1) // align * align == c_size == C.sizeof(lr.rt_denoise_variance) == 32
    assert int(align_attr or 8) == 8                           # the attribute names the natural alignment: no effect


def test_entry_points_are_declared_and_exported():
    names = lr.header_functions()
    assert "rt_denoise_var" in names and "rt_denoise_var_device" in names
    assert hasattr(lr.lib, "rt_denoise_var") and hasattr(lr.lib, "rt_denoise_var_device")
    assert lr.RT_ABI_VERSION == 10 == lr.lib.rt_abi_version()
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(lr.rt_denoise_variance) == 2 * ptr + 16
    assert (lr.rt_denoise_variance.variance.offset, lr.rt_denoise_variance.out_variance.offset) == (0, ptr)
    assert (lr.rt_denoise_variance.sigma_variance.offset, lr.rt_denoise_variance.variance_floor.offset) == (2 * ptr, 2 * ptr + 8)
    assert C.sizeof(lr.rt_denoise_params) == 48 and C.sizeof(lr.rt_denoise_inputs) == 4 * ptr      # as they were
    assert "aa_wavefront" == lr.tuning_keys()[-1]             # no new tuning key
    # a null context is refused before anything is touched
    p, i, v = lr.denoise_params(8, 8), lr.rt_denoise_inputs(), lr.rt_denoise_variance()
    assert lr.lib.rt_denoise_var(None, C.byref(p), C.byref(i), C.byref(v), None, None) == lr.RT_E_INVALID
    assert lr.lib.rt_denoise_var_device(None, C.byref(p), C.byref(i), C.byref(v), None, None, None) == lr.RT_E_INVALID
