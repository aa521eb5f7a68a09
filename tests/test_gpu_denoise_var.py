"""The device's variance-guided denoiser (rt_denoise_var / rt_denoise_var_device, the kVar kernels of
csrc/wf_denoise.hip) against the numpy model (tests/denoise_var_model.py, pinned on the CPU by
test_denoise_var_model.py): no tolerance.  The f32 colours and the f32 variance must have the model's bits
(non-finite values by position) and the BGR bytes must be the model's, on images smaller than a tile, larger than
several, narrower than the filter's reach, with every flag mask, 1 to 8 passes, both kernel forms, and the special
values the rule makes promises about -- in the colours, the guides and the variance image.
"""
import contextlib
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libraytrace as lr
from libraytrace import scenes

import denoise_model as dm
import denoise_var_model as dv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rust-raytrace_amd", "raytrace")
LINE = re.compile(r"rtamd: denoise-var (\d+)x(\d+) iters (\d+) flags 0x([0-9a-f]+) variant (\d+)")
PLAIN_LINE = re.compile(r"rtamd: denoise (\d+)x(\d+)")
# (width, height): one pixel; smaller than the kernel; a column strip; steps 16 and 32 beyond the image; several
# workgroup tiles (64 x 8) in both directions with ragged edges: the halo and the 3 x 3 prefilter reach tile and image
# borders
SIZES = [(1, 1), (5, 3), (3, 40), (37, 29), (70, 66)]
SETTINGS = dict(normal_squarings=2, sigma_color=0.7, sigma_depth=0.3, sigma_variance=1.5, variance_floor=2.0 ** -12)


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


@pytest.fixture(scope="module")
def images():
    """{(w, h, special): (rgb, normal, depth, albedo, variance)}, made once and never written."""
    out = {}
    for i, (w, h) in enumerate(SIZES):
        for special in (False, True):
            out[(w, h, special)] = dm.random_image(h, w, 100 + 2 * i + special, special) + (
                dv.random_variance(h, w, 200 + 2 * i + special, special),)
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out


_models = {}


def model_of(img, key, **kw):
    """The model of one image and one set of settings, computed once."""
    k = (key, tuple(sorted(kw.items())))
    if k not in _models:
        _models[k] = dv.denoise_var(img[0], img[4], img[1], img[2], img[3], **kw)
    return _models[k]


def guides_of(img):
    return {"normal": img[1], "depth": img[2], "albedo": img[3]}


def same(got_rgb, got_bgr, got_var, model, what):
    if got_rgb is not None:
        assert got_rgb.shape == model["rgb"].shape, what
        bad = ~dm.om.same_f32(got_rgb, model["rgb"])
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got_rgb[bad][:4], model["rgb"][bad][:4])
    if got_bgr is not None:
        w = model["rgb"].shape[1]
        bad = got_bgr[:, :3 * w] != model["bgr"][:, :3 * w]
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    if got_var is not None:
        assert got_var.shape == model["variance"].shape, what
        bad = got_var.view(np.uint32) != model["variance"].view(np.uint32)        # never NaN: every bit
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got_var[bad][:4], model["variance"][bad][:4])


def check(ctx, img, key, what="", **kw):
    kw = dict(SETTINGS, **kw)
    rgb, bgr, var = ctx.denoise_var(img[0], img[4], guides_of(img), variance_out=True, **kw)
    model = model_of(img, key, **{k: v for k, v in kw.items() if k != "variant"})
    same(rgb, bgr, var, model, (what, kw))
    return rgb, bgr, var


@pytest.mark.parametrize("size", SIZES)
def test_sizes_iterations_and_masks(gpu_ctx, images, size):
    key = size + (False,)
    for iterations, flags in ((1, 15), (2, 3), (5, 7), (8, 15), (8, 0)):
        for variant in (1, 2):
            check(gpu_ctx, images[key], key, size, iterations=iterations, flags=flags, variant=variant)


@pytest.mark.parametrize("flags", dv.ALL_MASKS)
def test_every_flag_mask(gpu_ctx, images, flags):
    check(gpu_ctx, images[(70, 66, False)], (70, 66, False), "mask", iterations=3, flags=flags)
    check(gpu_ctx, images[(37, 29, True)], (37, 29, True), "mask, special values", iterations=3, flags=flags)


@pytest.mark.parametrize("size", SIZES)
def test_special_values(gpu_ctx, images, size):
    """NaN and inf colours, NaN depths, zero normals and albedo channels, -0.0; a variance image with NaN, -1, -0.0, 0,
    +inf, f32 denormals and 2^100: the model's bits, the non-finite colours exactly where the input has them, and no
    variance NaN or negative."""
    key = size + (True,)
    img = images[key]
    for iterations, flags in ((1, 15), (4, 7), (5, 3)):
        for variant in (1, 2):
            rgb, _, var = check(gpu_ctx, img, key, size, iterations=iterations, flags=flags, variant=variant)
            assert np.array_equal(~np.isfinite(rgb), ~np.isfinite(img[0]))
            assert (var >= 0).all() and not np.signbit(var).any()


def test_all_forms_give_the_same_bits_and_say_which_ran(gpu_ctx, images, capfd):
    img = images[(70, 66, True)]
    got = {}
    with tuning(gpu_ctx, verbose=1):
        for variant in (0, 1, 2):
            capfd.readouterr()
            got[variant] = gpu_ctx.denoise_var(img[0], img[4], guides_of(img), variance_out=True, iterations=5, flags=15,
                                               variant=variant, **SETTINGS)
            err = capfd.readouterr().err
            lines = LINE.findall(err)
            assert len(lines) == 1 and not PLAIN_LINE.findall(err), err
            w, h, it, fl, v = (int(lines[0][0]), int(lines[0][1]), int(lines[0][2]), int(lines[0][3], 16), int(lines[0][4]))
            assert (w, h, it, fl) == (70, 66, 5, 15)
            assert v == variant if variant else v in (1, 2)
    capfd.readouterr()
    gpu_ctx.denoise_var(img[0], img[4], iterations=1, flags=0)
    assert not LINE.findall(capfd.readouterr().err)           # silent without tuning verbose
    for variant in (0, 2):
        for a, b in zip(got[variant], got[1]):
            assert a.tobytes() == b.tobytes()
    same(*got[1], model_of(img, (70, 66, True), iterations=5, flags=15, **SETTINGS), "variant 1")


def test_sigma_and_floor_reach_the_kernel(gpu_ctx, images):
    key = (70, 66, False)
    for sv, floor in ((0.25, 1e-6), (8.0, 0.5), (1e200, 1e-300), (1e-200, 1e300)):
        check(gpu_ctx, images[key], key, "sigma, floor", iterations=3, flags=3, sigma_variance=sv, variance_floor=floor)
    a = check(gpu_ctx, images[key], key, iterations=3, flags=3, sigma_variance=0.25, variance_floor=1e-6)
    b = check(gpu_ctx, images[key], key, iterations=3, flags=3, sigma_variance=8.0, variance_floor=0.5)
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[2], b[2])


def test_padded_rows_keep_their_bytes(gpu_ctx, images):
    for (w, h), pad in (((70, 66), 6), ((37, 29), 1), ((5, 3), 17)):
        key = (w, h, False)
        rgb, bgr, _ = check(gpu_ctx, images[key], key, "pitch", iterations=2, flags=3, bgr_pitch=3 * w + pad)
        assert bgr.shape == (h, 3 * w + pad) and (bgr[:, 3 * w:] == 0xCD).all()


def test_one_output_at_a_time(gpu_ctx, images):
    key = (70, 66, False)
    img = images[key]
    kw = dict(SETTINGS, iterations=3, flags=15)
    model = model_of(img, key, **kw)
    rgb, bgr, var = gpu_ctx.denoise_var(img[0], img[4], guides_of(img), bgr_out=False, **kw)
    assert bgr is None and var is None
    same(rgb, None, None, model, "rgb only")
    rgb, bgr, var = gpu_ctx.denoise_var(img[0], img[4], guides_of(img), rgb_out=False, **kw)
    assert rgb is None and var is None
    same(None, bgr, None, model, "bgr only")
    rgb, bgr, var = gpu_ctx.denoise_var(img[0], img[4], guides_of(img), rgb_out=False, bgr_out=False, variance_out=True, **kw)
    assert rgb is None and bgr is None
    same(None, None, var, model, "variance only")


def test_out_variance_between_guard_floats(gpu_ctx, images):
    """The host variant copies out_variance back as w * h floats and nothing around them."""
    for key in ((70, 66, False), (37, 29, True), (1, 1, False)):
        w, h = key[:2]
        img = images[key]
        kw = dict(SETTINGS, iterations=2, flags=7)
        guard = 16
        buf = np.full(guard + w * h + guard, -123.0, np.float32)
        out_rgb = np.zeros((h, w, 3), np.float32)
        p = lr.denoise_params(w, h, **{k: v for k, v in kw.items() if k not in ("sigma_variance", "variance_floor")})
        ins = lr.rt_denoise_inputs(rgb=img[0].ctypes.data, normal=img[1].ctypes.data, depth=img[2].ctypes.data,
                                   albedo=img[3].ctypes.data)
        var = lr.rt_denoise_variance(variance=img[4].ctypes.data, out_variance=buf.ctypes.data + 4 * guard,
                                     sigma_variance=kw["sigma_variance"], variance_floor=kw["variance_floor"])
        assert lr.lib.rt_denoise_var(gpu_ctx._h, C.byref(p), C.byref(ins), C.byref(var), out_rgb.ctypes.data, None) == lr.RT_OK
        assert (buf[:guard] == -123.0).all() and (buf[-guard:] == -123.0).all()
        same(out_rgb, None, buf[guard:-guard].reshape(h, w), model_of(img, key, **kw), ("guards", key))


@pytest.mark.parametrize("flags", dv.ALL_MASKS)
def test_huge_variance_gives_the_plain_filters_bits_on_the_device(gpu_ctx, images, flags):
    """Variance 2^100 everywhere: every new divisor is 1.0, and Context.denoise's own output comes back."""
    img = images[(70, 66, False)]
    var = np.full((66, 70, 3), 2.0 ** 100, np.float32)
    kw = dict(iterations=5, flags=flags, normal_squarings=2, sigma_color=0.7, sigma_depth=0.3)
    for variant in (1, 2):
        plain = gpu_ctx.denoise(img[0], guides_of(img), variant=variant, **kw)
        rgb, bgr, out_var = gpu_ctx.denoise_var(img[0], var, guides_of(img), variance_out=True, variant=variant, **kw)
        assert rgb.tobytes() == plain[0].tobytes() and bgr.tobytes() == plain[1].tobytes()
        assert np.isfinite(out_var).all() and (out_var > 0).all()


def test_needs_no_scene_and_leaves_the_statistics_alone(gpu_ctx, images):
    key = (37, 29, False)
    with lr.Context(0) as fresh:                              # nothing uploaded
        check(fresh, images[key], key, "no scene", iterations=2, flags=3)
    spec = scenes.config3(48, 32, n=40)
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    gpu_ctx.render(lr.render_opts(48, 32, max_depth=3, spp=1))
    before, gens = gpu_ctx.stats(), gpu_ctx.generation_counts()
    check(gpu_ctx, images[key], key, "after a render", iterations=2, flags=3)
    after = gpu_ctx.stats()
    for name, _ in lr.rt_stats._fields_:
        assert getattr(before, name) == getattr(after, name), name
    assert before.rays > 0 and np.array_equal(gens[0], gpu_ctx.generation_counts()[0])
    assert np.array_equal(gens[1], gpu_ctx.generation_counts()[1])


def test_every_refusal(gpu_ctx, images):
    key = (37, 29, False)
    img = images[key]
    w, h = 37, 29
    gpu_ctx.upload(lr.Scene.deserialize(scenes.config3(48, 32, n=40).to_text()))
    gpu_ctx.render(lr.render_opts(48, 32, max_depth=3, spp=1))
    before = gpu_ctx.stats()
    out_rgb, out_bgr = np.full((h, w, 3), 7.0, np.float32), np.full((h, 3 * w), 0xCD, np.uint8)
    out_var = np.full((h, w), 7.0, np.float32)
    P = lambda a: a.ctypes.data                               # noqa: E731

    def params(**kw):
        return lr.denoise_params(w, h, **dict(dict(iterations=3, flags=15, normal_squarings=2, sigma_color=0.7, sigma_depth=0.3), **kw))

    def inputs(**kw):
        return lr.rt_denoise_inputs(**dict(dict(rgb=P(img[0]), normal=P(img[1]), depth=P(img[2]), albedo=P(img[3])), **kw))

    def variance(**kw):
        return lr.rt_denoise_variance(**dict(dict(variance=P(img[4]), out_variance=P(out_var), sigma_variance=2.0,
                                                  variance_floor=2.0 ** -20), **kw))

    def refused(p, i, v, rgb=P(out_rgb), bgr=P(out_bgr), word=""):
        for call in (lambda: lr.lib.rt_denoise_var(gpu_ctx._h, p, i, v, rgb, bgr),
                     lambda: lr.lib.rt_denoise_var_device(gpu_ctx._h, p, i, v, rgb, bgr, None)):
            assert call() == lr.RT_E_INVALID, word
            text = lr.lib.rt_last_error(gpu_ctx._h).decode()
            assert word in text and "rt_denoise_var:" in text, (word, text)   # under the name of the entry point called

    good = C.byref(variance())
    # rt_denoise's refusals, in its order
    refused(None, C.byref(inputs()), good, word="null")
    refused(C.byref(params()), None, good, word="null")
    for kw, word in ((dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(flags=16), "flag"),
                     (dict(flags=15 | 1 << 20), "flag"), (dict(normal_squarings=11), "normal_squarings"), (dict(variant=3), "variant"),
                     (dict(sigma_depth=0.0), "sigma_depth"), (dict(sigma_depth=-1.0), "sigma_depth"),
                     (dict(sigma_depth=float("inf")), "sigma_depth"), (dict(sigma_depth=float("nan")), "sigma_depth"),
                     (dict(sigma_color=0.0), "sigma_color"), (dict(sigma_color=float("nan")), "sigma_color"),
                     (dict(sigma_color=float("inf")), "sigma_color"), (dict(bgr_pitch=3 * w - 1), "bgr_pitch")):
        refused(C.byref(params(**kw)), C.byref(inputs()), good, word=word)
    p = params()
    p.width = 0
    refused(C.byref(p), C.byref(inputs()), good, word="width")
    p = params()
    p.height = 0
    refused(C.byref(p), C.byref(inputs()), good, word="height")
    for kw, word in ((dict(rgb=None), "rgb"), (dict(normal=None), "guide"), (dict(depth=None), "guide"), (dict(albedo=None), "guide")):
        refused(C.byref(params()), C.byref(inputs(**kw)), good, word=word)
    refused(C.byref(params()), C.byref(inputs()), C.byref(variance(out_variance=None)), rgb=None, bgr=None, word="three outputs")
    refused(C.byref(params()), C.byref(inputs()), None, rgb=None, bgr=None, word="three outputs")
    refused(C.byref(params()), C.byref(inputs()), good, rgb=P(img[0]), word="out_rgb")
    # then the struct's
    refused(C.byref(params()), C.byref(inputs()), None, word="rt_denoise_variance")
    refused(C.byref(params()), C.byref(inputs()), C.byref(variance(variance=None)), word="variance input")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(C.byref(params()), C.byref(inputs()), C.byref(variance(sigma_variance=bad)), word="sigma_variance")
        refused(C.byref(params()), C.byref(inputs()), C.byref(variance(variance_floor=bad)), word="variance_floor")
    refused(C.byref(params()), C.byref(inputs()), C.byref(variance(out_variance=P(img[4]))), word="out_variance")
    # the order: rt_denoise's checks before the struct's, the struct's in the header's order
    refused(C.byref(params(variant=3)), C.byref(inputs()), C.byref(variance(variance=None, sigma_variance=0.0)), word="variant")
    refused(C.byref(params()), C.byref(inputs()), C.byref(variance(variance=None, sigma_variance=0.0)), word="variance input")
    refused(C.byref(params()), C.byref(inputs()), C.byref(variance(sigma_variance=0.0, variance_floor=0.0)), word="sigma_variance")
    # nothing changed: the outputs, the statistics, and the next good call
    assert (out_rgb == 7.0).all() and (out_bgr == 0xCD).all() and (out_var == 7.0).all()
    after = gpu_ctx.stats()
    assert all(getattr(before, n) == getattr(after, n) for n, _ in lr.rt_stats._fields_)
    check(gpu_ctx, img, key, "after the refusals", iterations=2, flags=3)
    # out_variance alone is an output; a guide that is not selected may be NULL
    rgb, bgr, var = gpu_ctx.denoise_var(img[0], img[4], {"normal": img[1]}, rgb_out=False, bgr_out=False, variance_out=True,
                                        iterations=2, flags=dm.NORMAL, normal_squarings=1, sigma_color=-1.0, sigma_depth=float("nan"))
    same(None, None, var, dv.denoise_var(img[0], img[4], img[1], iterations=2, flags=dm.NORMAL, normal_squarings=1), "unselected guides")


# ---- rt_denoise_var_device on torch streams ------------------------------------------------------

_DEVICE = r"""
import sys
sys.path[:0] = sys.argv[1:4]
import numpy as np
import torch                      # first: the process then uses torch's HIP runtime for both
import libraytrace as lr
from libraytrace import scenes
import denoise_model as dm
import denoise_var_model as dv

dev = torch.device("cuda", 0)
s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)       # not torch's default stream
assert s1.cuda_stream != 0 and s2.cuda_stream != 0 and s1.cuda_stream != s2.cuda_stream
KW = dict(iterations=5, flags=15, normal_squarings=2, sigma_color=0.7, sigma_depth=0.3)
VKW = dict(sigma_variance=1.5, variance_floor=2.0 ** -12)
GUARD = 32


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same(rgb, bgr, var, model, what):
    assert bool(dm.om.same_f32(rgb, model["rgb"]).all()), what
    assert np.array_equal(bgr, model["bgr"]), what
    if var is not None:
        assert np.array_equal(var.view(np.uint32), model["variance"].view(np.uint32)), what


def run_plain(ctx, t, w, h, stream):
    out_rgb = torch.full((h, w, 3), -7.0, dtype=torch.float32, device=dev)
    out_bgr = torch.full((h, 3 * w), 0xCD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.denoise_device(lr.denoise_params(w, h, **KW), t[0].data_ptr(),
                       {"normal": t[1].data_ptr(), "depth": t[2].data_ptr(), "albedo": t[3].data_ptr()},
                       out_rgb.data_ptr(), out_bgr.data_ptr(), stream.cuda_stream)
    return out_rgb, out_bgr


def run_var(ctx, t, w, h, stream, pitch=0, kw=KW):
    out_rgb = torch.full((h, w, 3), -7.0, dtype=torch.float32, device=dev)
    out_bgr = torch.full((h, pitch or 3 * w), 0xCD, dtype=torch.uint8, device=dev)
    out_var = torch.full((GUARD + h * w + GUARD,), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.denoise_var_device(lr.denoise_params(w, h, bgr_pitch=pitch, **kw), t[0].data_ptr(), t[4].data_ptr(),
                           {"normal": t[1].data_ptr(), "depth": t[2].data_ptr(), "albedo": t[3].data_ptr()},
                           out_rgb.data_ptr(), out_bgr.data_ptr(), out_var.data_ptr() + 4 * GUARD, stream_ptr=stream.cuda_stream,
                           **VKW)
    return out_rgb, out_bgr, out_var


def var_of(out_var, w, h):
    v = out_var.cpu().numpy()
    assert (v[:GUARD] == -7.0).all() and (v[-GUARD:] == -7.0).all(), "guard floats around out_variance"
    return v[GUARD:-GUARD].reshape(h, w)


with lr.Context(0) as ctx:
    # device buffers on a torch stream, padded rows: the sentinels stay, and the floats around out_variance
    w, h = 70, 66
    a = dm.random_image(h, w, 41, True) + (dv.random_variance(h, w, 43, True),)
    b = dm.random_image(h, w, 42, False) + (dv.random_variance(h, w, 44, False),)
    ta, tb = [up(x) for x in a], [up(x) for x in b]
    ma = dv.denoise_var(a[0], a[4], a[1], a[2], a[3], **KW, **VKW)
    mb = dv.denoise_var(b[0], b[4], b[1], b[2], b[3], **KW, **VKW)
    plain_b = dm.denoise(*b[:4], **KW)
    rgb, bgr, var = run_var(ctx, ta, w, h, s1, pitch=3 * w + 10)
    s1.synchronize()
    bgr = bgr.cpu().numpy()
    same(rgb.cpu().numpy(), bgr[:, :3 * w], var_of(var, w, h), ma, "padded")
    assert (bgr[:, 3 * w:] == 0xCD).all()
    # a plain denoise and a variance-guided one back to back on two streams share the scratch: each gives what it
    # gives alone, in either order
    for _ in range(2):
        ra, ba, va = run_var(ctx, ta, w, h, s1)
        rb, bb = run_plain(ctx, tb, w, h, s2)
        rc, bc, vc = run_var(ctx, tb, w, h, s1)
        s1.synchronize(); s2.synchronize()
        same(ra.cpu().numpy(), ba.cpu().numpy(), var_of(va, w, h), ma, "guided, then plain")
        same(rb.cpu().numpy(), bb.cpu().numpy(), None, plain_b, "plain between two guided")
        same(rc.cpu().numpy(), bc.cpu().numpy(), var_of(vc, w, h), mb, "guided after plain")
    # end to end: moments accumulate -> the variance on the device -> feature buffers -> the filter, all on one stream
    spec = scenes.stochastic(96, 64)
    W, H = spec.width, spec.height
    ctx.upload(lr.Scene.deserialize(spec.to_text()))
    o = lr.render_opts(W, H, max_depth=spec.max_depth, spp=4, jitter=1, seed=7, flags=lr.RT_OUT_RGB_F32)
    t = [torch.zeros((H, W, 3), dtype=torch.float32, device=dev), torch.zeros((H, W, 3), dtype=torch.float32, device=dev),
         torch.zeros((H, W), dtype=torch.float32, device=dev), torch.zeros((H, W, 3), dtype=torch.float32, device=dev),
         torch.zeros((H, W, 3), dtype=torch.float32, device=dev)]
    torch.cuda.synchronize(dev)
    with ctx.accumulator(o, moments=True) as acc:
        acc.add(4, stream_ptr=s1.cuda_stream)
        acc.resolve_device(t[0].data_ptr(), 0, stream_ptr=s1.cuda_stream)
        acc.noise_device(1e-3, 1.0, t[4].data_ptr(), None, s1.cuda_stream)
        ctx.render_aov_device(o, lr.RT_AOV_NORMAL | lr.RT_AOV_DEPTH | lr.RT_AOV_ALBEDO,
                              {"normal": t[1].data_ptr(), "depth": t[2].data_ptr(), "albedo": t[3].data_ptr()}, s1.cuda_stream)
        pipe = dict(iterations=5, flags=3, normal_squarings=5, sigma_color=1.0, sigma_depth=0.05)
        rgb, bgr, var = run_var(ctx, t, W, H, s1, kw=pipe)
        s1.synchronize()
    host = [x.cpu().numpy() for x in t]
    assert all(x.any() for x in host)
    one_shot, _, _ = ctx.render(o, bgr=False)
    assert one_shot.tobytes() == host[0].tobytes()            # one accumulate call: the one-shot render's bits
    model = dv.denoise_var(host[0], host[4], host[1], host[2], host[3], **pipe, **VKW)
    same(rgb.cpu().numpy(), bgr.cpu().numpy(), var_of(var, W, H), model, "end to end")
    assert not np.array_equal(rgb.cpu().numpy(), host[0])
print("denoise_var_device ok")
"""


def test_device_buffers_on_torch_streams():
    """In a child process: torch must initialise HIP before the library does."""
    out = subprocess.run([sys.executable, "-c", _DEVICE, ROOT, os.path.join(ROOT, "rust-raytrace_amd"),
                          os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "denoise_var_device ok" in out.stdout, out.stderr[-3000:]


# ---- the CLI -------------------------------------------------------------------------------------

def test_cli_writes_the_variance_guided_image(gpu_ctx, tmp_path):
    spec = scenes.stochastic(96, 64)                          # 3 * 96 is a multiple of 4: BMP rows without padding
    scene = tmp_path / "scene.txt"
    scene.write_text(spec.to_text())
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    o = lr.render_opts(96, 64, max_depth=4, spp=4, jitter=1, seed=7)
    with gpu_ctx.accumulator(o, moments=True) as acc:
        acc.add(4)
        rgb, _ = acc.resolve(bgr=False)
        var, _, _ = acc.noise(1e-3, 1.0, error=False)
    g, _ = gpu_ctx.render_aov(o, lr.RT_AOV_NORMAL | lr.RT_AOV_DEPTH | lr.RT_AOV_ALBEDO)
    header, pitch = lr.bmp_header(96, 64)
    assert pitch == 288
    base = [EXE, "--scene", str(scene), "--spp", "4", "--jitter", "random", "--seed", "7", "--denoise", "5"]
    for extra, kw in ((["--denoise-variance", "2"], dict(sigma_variance=2.0)),
                      (["--denoise-variance", "3", "--denoise-variance-floor", "0.001", "--progressive", "2"],
                       dict(sigma_variance=3.0, variance_floor=0.001))):
        out = tmp_path / "out.bmp"
        run = subprocess.run(base + ["--out", str(out)] + extra, capture_output=True, text=True, timeout=100)
        assert run.returncode == 0, run.stdout + run.stderr
        _, bgr, _ = gpu_ctx.denoise_var(rgb, var, g, rgb_out=False, iterations=5, flags=3, normal_squarings=5, sigma_color=1.0,
                                        sigma_depth=0.05, **kw)
        assert out.read_bytes() == bytes(header) + bgr.tobytes(), extra
        out.unlink()
    # --progressive 1: the frame of 1 sample has no variance and says so; the last frame is the same image
    out = tmp_path / "out.bmp"
    run = subprocess.run(base + ["--out", str(out), "--denoise-variance", "2", "--progressive", "1"], capture_output=True, text=True,
                         timeout=100)
    assert run.returncode == 0 and "plain filter" in run.stderr, run.stdout + run.stderr
    _, bgr, _ = gpu_ctx.denoise_var(rgb, var, g, rgb_out=False, iterations=5, flags=3, normal_squarings=5, sigma_color=1.0,
                                    sigma_depth=0.05, sigma_variance=2.0)
    assert out.read_bytes() == bytes(header) + bgr.tobytes()
    # --variance beside it writes the image the filter was guided by; the BMP is the same
    pfm = tmp_path / "var.pfm"
    run = subprocess.run(base + ["--out", str(out), "--denoise-variance", "2", "--variance", str(pfm)], capture_output=True, text=True,
                         timeout=100)
    assert run.returncode == 0, run.stdout + run.stderr
    assert out.read_bytes() == bytes(header) + bgr.tobytes()
    assert pfm.read_bytes().endswith(var.tobytes()) and len(pfm.read_bytes()) - var.nbytes < 32
    # refused with a message: a jitter that is not random, --spp below 2, more than one device, no --denoise, a
    # DepthOfField camera (no feature buffers)
    for extra, word in ((["--jitter", "center"], "--jitter random"), (["--spp", "1"], "--spp"), (["--gpus", "2"], "--gpus"),
                        (["--denoise-variance-floor", "0"], "--denoise-variance-floor")):
        run = subprocess.run(base + ["--out", str(tmp_path / "no.bmp"), "--denoise-variance", "2"] + extra, capture_output=True,
                             text=True, timeout=100)
        assert run.returncode == 2 and word in run.stdout, (extra, run.stdout + run.stderr)
    run = subprocess.run([EXE, "--scene", str(scene), "--out", str(tmp_path / "no.bmp"), "--denoise-variance", "2"],
                         capture_output=True, text=True, timeout=100)
    assert run.returncode == 2 and "--denoise ITER" in run.stdout, run.stdout + run.stderr
    dof = tmp_path / "dof.txt"
    dof.write_text(scenes.stochastic(48, 32, dof=True).to_text())
    run = subprocess.run([EXE, "--scene", str(dof), "--out", str(tmp_path / "no.bmp"), "--spp", "4", "--denoise", "2",
                          "--denoise-variance", "2"], capture_output=True, text=True, timeout=100)
    assert run.returncode == 2 and "--denoise" in run.stdout and "DepthOfField" in run.stdout, run.stdout + run.stderr
    assert not (tmp_path / "no.bmp").exists()
