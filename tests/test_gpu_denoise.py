"""The device's denoiser (rt_denoise / rt_denoise_device, csrc/wf_denoise.hip) against the numpy model
(tests/denoise_model.py, pinned on the CPU by test_denoise_model.py): no tolerance.  The f32 output must have the
model's bits (non-finite values by position) and the BGR bytes must be the model's, on images smaller than a tile,
larger than several, narrower than the filter's reach, with every flag mask, 1 to 8 passes, both kernel forms, and
the special values the rule makes promises about.
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rust-raytrace_amd", "raytrace")
LINE = re.compile(r"rtamd: denoise (\d+)x(\d+) iters (\d+) flags 0x([0-9a-f]+) variant (\d+)")
# (width, height): one pixel; smaller than the kernel; a column strip; steps 16 and 32 beyond the image; several
# workgroup tiles (64 x 8) in both directions with ragged edges
SIZES = [(1, 1), (5, 3), (3, 40), (37, 29), (70, 66)]
SETTINGS = dict(normal_squarings=2, sigma_color=0.7, sigma_depth=0.3)


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
    """{(w, h, special): (rgb, normal, depth, albedo)}, made once and never written."""
    out = {}
    for i, (w, h) in enumerate(SIZES):
        for special in (False, True):
            out[(w, h, special)] = dm.random_image(h, w, 100 + 2 * i + special, special)
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out


def guides_of(img):
    return {"normal": img[1], "depth": img[2], "albedo": img[3]}


def same(got_rgb, got_bgr, model, what):
    if got_rgb is not None:
        assert got_rgb.shape == model["rgb"].shape, what
        bad = ~dm.om.same_f32(got_rgb, model["rgb"])
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got_rgb[bad][:4], model["rgb"][bad][:4])
    if got_bgr is not None:
        w = model["rgb"].shape[1]
        bad = got_bgr[:, :3 * w] != model["bgr"][:, :3 * w]
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def check(ctx, img, what="", **kw):
    kw = dict(SETTINGS, **kw)
    rgb, bgr = ctx.denoise(img[0], guides_of(img), **kw)
    model = dm.denoise(*img, **{k: v for k, v in kw.items() if k != "variant"})
    same(rgb, bgr, model, (what, kw))
    return rgb, bgr


@pytest.mark.parametrize("size", SIZES)
def test_sizes_iterations_and_masks(gpu_ctx, images, size):
    img = images[size + (False,)]
    for iterations, flags in ((1, 15), (2, 3), (5, 7), (8, 15), (8, 0)):
        for variant in (1, 2):
            check(gpu_ctx, img, size, iterations=iterations, flags=flags, variant=variant)


@pytest.mark.parametrize("flags", dm.ALL_MASKS)
def test_every_flag_mask(gpu_ctx, images, flags):
    check(gpu_ctx, images[(70, 66, False)], "mask", iterations=3, flags=flags)
    check(gpu_ctx, images[(37, 29, True)], "mask, special values", iterations=3, flags=flags)


@pytest.mark.parametrize("size", SIZES)
def test_special_values(gpu_ctx, images, size):
    """NaN and inf colours, NaN depths, zero normals, zero albedo channels, -0.0: the model's bits, and the non-finite
    values exactly where the input has them."""
    img = images[size + (True,)]
    for iterations, flags in ((1, 15), (4, 7), (5, 3)):
        for variant in (1, 2):
            rgb, _ = check(gpu_ctx, img, size, iterations=iterations, flags=flags, variant=variant)
            assert np.array_equal(~np.isfinite(rgb), ~np.isfinite(img[0]))


def test_both_forms_give_the_same_bits_and_say_which_ran(gpu_ctx, images, capfd):
    img = images[(70, 66, True)]
    got = {}
    with tuning(gpu_ctx, verbose=1):
        for variant in (0, 1, 2):
            capfd.readouterr()
            got[variant] = gpu_ctx.denoise(img[0], guides_of(img), iterations=5, flags=15, variant=variant, **SETTINGS)
            lines = LINE.findall(capfd.readouterr().err)
            assert len(lines) == 1, lines
            w, h, it, fl, v = (int(lines[0][0]), int(lines[0][1]), int(lines[0][2]), int(lines[0][3], 16), int(lines[0][4]))
            assert (w, h, it, fl) == (70, 66, 5, 15)
            assert v == variant if variant else v in (1, 2)
    capfd.readouterr()
    gpu_ctx.denoise(img[0], guides_of(img), iterations=1, flags=0)
    assert not LINE.findall(capfd.readouterr().err)           # silent without tuning verbose
    for variant in (0, 2):
        assert got[variant][0].tobytes() == got[1][0].tobytes() and got[variant][1].tobytes() == got[1][1].tobytes()


@pytest.mark.parametrize("squarings", [0, 10])
def test_normal_squarings(gpu_ctx, images, squarings):
    for key in ((70, 66, False), (37, 29, True)):
        check(gpu_ctx, images[key], "squarings", iterations=3, flags=dm.NORMAL | dm.COLOR, normal_squarings=squarings)


def test_padded_rows_keep_their_bytes(gpu_ctx, images):
    for (w, h), pad in (((70, 66), 6), ((37, 29), 1), ((5, 3), 17), ((64, 8), 64)):
        img = images.get((w, h, False)) or dm.random_image(h, w, 7)
        rgb, bgr = check(gpu_ctx, img, "pitch", iterations=2, flags=3, bgr_pitch=3 * w + pad)
        assert bgr.shape == (h, 3 * w + pad) and (bgr[:, 3 * w:] == 0xCD).all()


def test_one_output_at_a_time(gpu_ctx, images):
    img = images[(70, 66, False)]
    model = dm.denoise(*img, iterations=3, flags=15, **SETTINGS)
    rgb, none = gpu_ctx.denoise(img[0], guides_of(img), bgr_out=False, iterations=3, flags=15, **SETTINGS)
    assert none is None
    same(rgb, None, model, "rgb only")
    none, bgr = gpu_ctx.denoise(img[0], guides_of(img), rgb_out=False, iterations=3, flags=15, **SETTINGS)
    assert none is None
    same(None, bgr, model, "bgr only")


def test_bgr_alone_into_padded_rows(gpu_ctx):
    """The host variant's pitched copy with no f32 output beside it: the model's bytes, and the padding untouched."""
    for (w, h), pad in (((8, 6), 5), ((5, 3), 1)):
        img = dm.random_image(h, w, 11)
        kw = dict(SETTINGS, iterations=2, flags=15, bgr_pitch=3 * w + pad)
        none, bgr = gpu_ctx.denoise(img[0], guides_of(img), rgb_out=False, **kw)
        assert none is None and bgr.shape == (h, 3 * w + pad)
        same(None, bgr, dm.denoise(*img, **kw), ("bgr only, padded", w, h))
        assert (bgr[:, 3 * w:] == 0xCD).all()


def test_needs_no_scene_and_leaves_the_statistics_alone(gpu_ctx, images):
    img = images[(37, 29, False)]
    with lr.Context(0) as fresh:                              # nothing uploaded
        check(fresh, img, "no scene", iterations=2, flags=3)
    spec = scenes.config3(48, 32, n=40)
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    gpu_ctx.render(lr.render_opts(48, 32, max_depth=3, spp=1))
    before, gens = gpu_ctx.stats(), gpu_ctx.generation_counts()
    check(gpu_ctx, img, "after a render", iterations=2, flags=3)
    after = gpu_ctx.stats()
    for name, _ in lr.rt_stats._fields_:
        assert getattr(before, name) == getattr(after, name), name
    assert before.rays > 0 and np.array_equal(gens[0], gpu_ctx.generation_counts()[0])
    assert np.array_equal(gens[1], gpu_ctx.generation_counts()[1])


def test_every_refusal(gpu_ctx, images):
    img = images[(37, 29, False)]
    w, h = 37, 29
    gpu_ctx.upload(lr.Scene.deserialize(scenes.config3(48, 32, n=40).to_text()))
    gpu_ctx.render(lr.render_opts(48, 32, max_depth=3, spp=1))
    before = gpu_ctx.stats()
    out_rgb, out_bgr = np.full((h, w, 3), 7.0, np.float32), np.full((h, 3 * w), 0xCD, np.uint8)
    P = lambda a: a.ctypes.data                               # noqa: E731

    def params(**kw):
        return lr.denoise_params(w, h, **dict(dict(iterations=3, flags=15, normal_squarings=2, sigma_color=0.7, sigma_depth=0.3), **kw))

    def inputs(**kw):
        return lr.rt_denoise_inputs(**dict(dict(rgb=P(img[0]), normal=P(img[1]), depth=P(img[2]), albedo=P(img[3])), **kw))

    def refused(p, i, rgb=P(out_rgb), bgr=P(out_bgr), word=""):
        for call in (lambda: lr.lib.rt_denoise(gpu_ctx._h, p, i, rgb, bgr),
                     lambda: lr.lib.rt_denoise_device(gpu_ctx._h, p, i, rgb, bgr, None)):
            assert call() == lr.RT_E_INVALID, word
            assert word in lr.lib.rt_last_error(gpu_ctx._h).decode(), (word, lr.lib.rt_last_error(gpu_ctx._h))

    refused(None, C.byref(inputs()), word="null")
    refused(C.byref(params()), None, word="null")
    for kw, word in ((dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(flags=16), "flag"),
                     (dict(flags=15 | 1 << 20), "flag"), (dict(normal_squarings=11), "normal_squarings"), (dict(variant=3), "variant"),
                     (dict(sigma_depth=0.0), "sigma_depth"), (dict(sigma_depth=-1.0), "sigma_depth"),
                     (dict(sigma_depth=float("inf")), "sigma_depth"), (dict(sigma_depth=float("nan")), "sigma_depth"),
                     (dict(sigma_color=0.0), "sigma_color"), (dict(sigma_color=float("nan")), "sigma_color"),
                     (dict(sigma_color=float("inf")), "sigma_color"), (dict(bgr_pitch=3 * w - 1), "bgr_pitch")):
        refused(C.byref(params(**kw)), C.byref(inputs()), word=word)
    p = params()
    p.width = 0
    refused(C.byref(p), C.byref(inputs()), word="width")
    p = params()
    p.height = 0
    refused(C.byref(p), C.byref(inputs()), word="height")
    for kw, word in ((dict(rgb=None), "rgb"), (dict(normal=None), "guide"), (dict(depth=None), "guide"), (dict(albedo=None), "guide")):
        refused(C.byref(params()), C.byref(inputs(**kw)), word=word)
    refused(C.byref(params()), C.byref(inputs()), rgb=None, bgr=None, word="outputs")
    refused(C.byref(params()), C.byref(inputs()), rgb=P(img[0]), word="out_rgb")
    # nothing changed: the outputs, the statistics, and the next good call
    assert (out_rgb == 7.0).all() and (out_bgr == 0xCD).all()
    after = gpu_ctx.stats()
    assert all(getattr(before, n) == getattr(after, n) for n, _ in lr.rt_stats._fields_)
    # a guide that is not selected may be NULL, a sigma that is not selected anything
    rgb, bgr = gpu_ctx.denoise(img[0], {"normal": img[1]}, iterations=2, flags=dm.NORMAL, normal_squarings=1, sigma_color=-1.0,
                               sigma_depth=float("nan"))
    same(rgb, bgr, dm.denoise(img[0], img[1], iterations=2, flags=dm.NORMAL, normal_squarings=1), "unselected guides")


# ---- rt_denoise_device on torch streams ----------------------------------------------------------

_DEVICE = r"""
import sys
sys.path[:0] = sys.argv[1:4]
import numpy as np
import torch                      # first: the process then uses torch's HIP runtime for both
import libraytrace as lr
from libraytrace import scenes
import denoise_model as dm

dev = torch.device("cuda", 0)
s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)       # not torch's default stream
assert s1.cuda_stream != 0 and s2.cuda_stream != 0 and s1.cuda_stream != s2.cuda_stream
KW = dict(iterations=5, flags=15, normal_squarings=2, sigma_color=0.7, sigma_depth=0.3)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same(rgb, bgr, model, what):
    assert bool(dm.om.same_f32(rgb, model["rgb"]).all()), what
    assert np.array_equal(bgr, model["bgr"]), what


def run(ctx, t, w, h, stream, pitch=0):
    out_rgb = torch.full((h, w, 3), -7.0, dtype=torch.float32, device=dev)
    out_bgr = torch.full((h, pitch or 3 * w), 0xCD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.denoise_device(lr.denoise_params(w, h, bgr_pitch=pitch, **KW), t[0].data_ptr(),
                       {"normal": t[1].data_ptr(), "depth": t[2].data_ptr(), "albedo": t[3].data_ptr()},
                       out_rgb.data_ptr(), out_bgr.data_ptr(), stream.cuda_stream)
    return out_rgb, out_bgr


with lr.Context(0) as ctx:
    # device buffers on a torch stream, padded rows: the sentinels stay
    w, h = 70, 66
    a = dm.random_image(h, w, 41, True)
    b = dm.random_image(h, w, 42, False)
    ta, tb = [up(x) for x in a], [up(x) for x in b]
    ma, mb = dm.denoise(*a, **KW), dm.denoise(*b, **KW)
    rgb, bgr = run(ctx, ta, w, h, s1, pitch=3 * w + 10)
    s1.synchronize()
    bgr = bgr.cpu().numpy()
    same(rgb.cpu().numpy(), bgr[:, :3 * w], ma, "padded")
    assert (bgr[:, 3 * w:] == 0xCD).all()
    # two denoises back to back on two streams share the scratch: each gives what it gives alone
    for _ in range(3):
        ra, ba = run(ctx, ta, w, h, s1)
        rb, bb = run(ctx, tb, w, h, s2)
        s1.synchronize(); s2.synchronize()
        same(ra.cpu().numpy(), ba.cpu().numpy(), ma, "first of two")
        same(rb.cpu().numpy(), bb.cpu().numpy(), mb, "second of two")
    # end to end: colours and feature buffers rendered on the device, filtered there
    spec = scenes.stochastic(96, 64)
    W, H = spec.width, spec.height
    ctx.upload(lr.Scene.deserialize(spec.to_text()))
    o = lr.render_opts(W, H, max_depth=spec.max_depth, spp=4, jitter=1, seed=7, flags=lr.RT_OUT_RGB_F32)
    t = [torch.zeros((H, W, 3), dtype=torch.float32, device=dev), torch.zeros((H, W, 3), dtype=torch.float32, device=dev),
         torch.zeros((H, W), dtype=torch.float32, device=dev), torch.zeros((H, W, 3), dtype=torch.float32, device=dev)]
    torch.cuda.synchronize(dev)
    ctx.render_device(o, t[0].data_ptr(), 0, s1.cuda_stream)
    ctx.render_aov_device(o, lr.RT_AOV_NORMAL | lr.RT_AOV_DEPTH | lr.RT_AOV_ALBEDO,
                          {"normal": t[1].data_ptr(), "depth": t[2].data_ptr(), "albedo": t[3].data_ptr()}, s1.cuda_stream)
    rgb, bgr = run(ctx, t, W, H, s1)
    s1.synchronize()
    host = [x.cpu().numpy() for x in t]
    assert host[0].any() and host[1].any() and host[2].any() and host[3].any()
    model = dm.denoise(*host, **KW)
    same(rgb.cpu().numpy(), bgr.cpu().numpy(), model, "end to end")
    assert not np.array_equal(rgb.cpu().numpy(), host[0])
print("denoise_device ok")
"""


def test_device_buffers_on_torch_streams():
    """In a child process: torch must initialise HIP before the library does."""
    out = subprocess.run([sys.executable, "-c", _DEVICE, ROOT, os.path.join(ROOT, "rust-raytrace_amd"),
                          os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "denoise_device ok" in out.stdout, out.stderr[-3000:]


# ---- the CLI -------------------------------------------------------------------------------------

def test_cli_writes_the_denoised_image(gpu_ctx, tmp_path):
    spec = scenes.stochastic(96, 64)                          # 3 * 96 is a multiple of 4: BMP rows without padding
    scene = tmp_path / "scene.txt"
    scene.write_text(spec.to_text())
    gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
    o = lr.render_opts(96, 64, max_depth=4, spp=4, jitter=1, seed=7)
    rgb, _, _ = gpu_ctx.render(o, bgr=False)
    g, _ = gpu_ctx.render_aov(o, lr.RT_AOV_NORMAL | lr.RT_AOV_DEPTH | lr.RT_AOV_ALBEDO)
    header, pitch = lr.bmp_header(96, 64)
    assert pitch == 288
    for extra, flags in (([], 3), (["--denoise-flags", "normal,depth,color,demodulate"], 15), (["--progressive", "2"], 3)):
        out = tmp_path / "out.bmp"
        run = subprocess.run([EXE, "--scene", str(scene), "--out", str(out), "--spp", "4", "--jitter", "random", "--seed", "7",
                              "--denoise", "5"] + extra, capture_output=True, text=True, timeout=100)
        assert run.returncode == 0, run.stdout + run.stderr
        _, bgr = gpu_ctx.denoise(rgb, g, rgb_out=False, iterations=5, flags=flags, normal_squarings=5, sigma_color=1.0,
                                 sigma_depth=0.05)
        assert out.read_bytes() == bytes(header) + bgr.tobytes(), extra
        out.unlink()
    # more than one device and a DepthOfField camera (no feature buffers) are refused with a message
    run = subprocess.run([EXE, "--scene", str(scene), "--denoise", "5", "--gpus", "2"], capture_output=True, text=True, timeout=100)
    assert run.returncode == 2 and "--denoise" in run.stdout, run.stdout + run.stderr
    run = subprocess.run([EXE, "--scene", str(scene), "--denoise", "9"], capture_output=True, text=True, timeout=100)
    assert run.returncode == 2 and "--denoise" in run.stdout, run.stdout + run.stderr
    dof = tmp_path / "dof.txt"
    dof.write_text(scenes.stochastic(48, 32, dof=True).to_text())
    run = subprocess.run([EXE, "--scene", str(dof), "--out", str(tmp_path / "dof.bmp"), "--denoise", "2"], capture_output=True,
                         text=True, timeout=100)
    assert run.returncode == 2 and "--denoise" in run.stdout and "DepthOfField" in run.stdout, run.stdout + run.stderr
    assert not (tmp_path / "dof.bmp").exists()
