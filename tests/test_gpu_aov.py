"""First-hit feature buffers on the device (rt_render_aov / rt_render_aov_device, csrc/wf_aov.hip) against
the Python model (tests/aov_model.py, pinned against the oracle by test_aov_model.py).

Required equal, with no tolerance: every f32 channel bit for bit (uint32 views; a NaN by its position: IEEE
leaves a NaN's sign and payload open, and the model's NaN comes from the host's 0/0), the object ids, and
rays / shadow_rays / pixels / traced_rays / chunks of rt_ctx_stats.  A last bit that differs is a finding
about the kernel, not a reason for a tolerance.
"""
import contextlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libraytrace as lr
from libraytrace import scenes

import aov_model as am

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rust-raytrace_amd", "raytrace")
AOV_LINE = re.compile(r"rtamd: aov src (\d+) spp (\d+) channels 0x([0-9a-f]+) pixels (\d+)")
FLOATS = ("depth", "normal", "albedo", "coverage")
NAMES = FLOATS + ("object",)
BIT = {"depth": lr.RT_AOV_DEPTH, "normal": lr.RT_AOV_NORMAL, "albedo": lr.RT_AOV_ALBEDO,
       "coverage": lr.RT_AOV_COVERAGE, "object": lr.RT_AOV_OBJECT}
CENTER, RANDOM = am.CENTER, am.RANDOM


@pytest.fixture(scope="module")
def specs(tmp_path_factory):
    d = tmp_path_factory.mktemp("aov_sky")
    paths = [str(d / f"f{k}.ppm") for k in range(6)]
    for p, f in zip(paths, scenes.skybox_faces(size=8, seed=2)):
        scenes.write_ppm(p, f)
    return am.scene_list(paths)


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


def opts(spec, spp, jitter, seed, **kw):
    # max_depth, algo, flags and bgr_pitch are ignored: values rt_render would refuse must not matter
    return lr.render_opts(spec.width, spec.height, spp=spp, jitter=jitter, seed=seed,
                          **dict(dict(max_depth=99, algo=77, bgr_pitch=1), **kw))


def render(ctx, capfd, spec, spp, jitter, seed, channels=lr.RT_AOV_ALL, out=None, **kw):
    """One rt_render_aov under tuning verbose -> (arrays, statistics, the source its verbose line names)."""
    o = opts(spec, spp, jitter, seed, **kw)
    with tuning(ctx, verbose=1):
        capfd.readouterr()
        arrays, st = ctx.render_aov(o, channels, out=out)
        err = capfd.readouterr().err
    lines = AOV_LINE.findall(err)
    assert len(lines) == 1, err
    src, lspp, lch, lpix = int(lines[0][0]), int(lines[0][1]), int(lines[0][2], 16), int(lines[0][3])
    assert (lspp, lch, lpix) == (spp, channels, o.tile_w * o.tile_h), err
    check_stats(st, o.tile_w * o.tile_h, spp, jitter)
    return arrays, st, src


def check_stats(st, pixels, spp, jitter):
    assert (st.rays, st.shadow_rays, st.pixels, st.chunks) == (pixels * spp, 0, pixels, 0), \
        (st.rays, st.shadow_rays, st.pixels, st.chunks)
    assert st.traced_rays == (pixels if jitter == CENTER else pixels * spp), st.traced_rays


def same(got, want, what=""):
    """Device arrays against the model's (or another render's): bits, NaN positions, ids."""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name in got:
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        if name == "object":
            assert np.array_equal(g, w), (what, name, int((g != w).sum()))
            continue
        ng, nw = np.isnan(g), np.isnan(w)
        assert np.array_equal(ng, nw), (what, name, "NaN mask", int(ng.sum()), int(nw.sum()))
        bad = am.bits(g)[~ng] != am.bits(w)[~nw]
        assert not bad.any(), (what, name, int(bad.sum()), g[~ng][bad][:4], w[~nw][bad][:4])


def sub(model, rows, cols):
    return {k: np.ascontiguousarray(v[rows][:, cols]) for k, v in model.items()}


def upload(ctx, spec):
    ctx.upload(lr.Scene.deserialize(spec.to_text()))


# ---- every scene, every case -------------------------------------------------------------------

@pytest.mark.parametrize("name", am.SCENE_NAMES)
def test_scene_matches_the_model(gpu_ctx, capfd, specs, name):
    spec = specs[name]
    upload(gpu_ctx, spec)
    for spp, jitter in am.CASES:
        for seed in (am.SEEDS if jitter == RANDOM else am.SEEDS[:1]):
            got, st, src = render(gpu_ctx, capfd, spec, spp, jitter, seed)
            same(got, am.aov(spec, spp, jitter, seed), (name, spp, jitter, seed, src))


def test_spp_zero_is_the_scenes_value(gpu_ctx, capfd, specs):
    spec = specs["stochastic"]                      # antialias 4
    upload(gpu_ctx, spec)
    o = opts(spec, 0, RANDOM, am.SEEDS[0])
    arrays, st = gpu_ctx.render_aov(o)
    check_stats(st, spec.width * spec.height, 4, RANDOM)
    same(arrays, am.aov(spec, 4, RANDOM, am.SEEDS[0]))


# ---- every source family -----------------------------------------------------------------------

SMALL = lambda: scenes.random_spheres(200, 64, 48, 4, seed=11, name="sources")                       # noqa: E731
BIG = lambda: scenes.random_spheres(2500, 64, 48, 4, seed=12, box_scale=2.0, name="sources_big")     # noqa: E731
# (scene, tuning) -> the source that must run; the sizes are test_gpu_sources.py's: 200 spheres fit LDS whole,
# 2500 do not (nor does their tree), and the prefix sources get a 1 KB prefix so that most of the tree is below it
FAMILIES = [
    ("small", dict(cam=3), 22), ("small", dict(cam=-1), 22),
    ("small", dict(cam=0), 9), ("small", dict(cam=0, src=9), 9), ("small", dict(cam=0, src=7), 7),
    ("small", dict(cam=0, src=2), 2), ("small", dict(cam=0, src=8, prefix_kb=1), 8),
    ("small", dict(cam=0, src=1), 1), ("small", dict(cam=0, src=0), 0),
    ("big", dict(cam=-1), 23), ("big", dict(cam=0, src=5, prefix_kb=1), 5), ("big", dict(cam=0, src=6, prefix_kb=1), 6),
    ("big", dict(cam=0, src=8, prefix_kb=1), 8), ("big", dict(cam=0, src=1), 0), ("big", dict(cam=0, src=2), 2),
]


@pytest.mark.parametrize("scene", ["small", "big"])
def test_every_source_family_agrees(gpu_ctx, capfd, scene):
    spec = SMALL() if scene == "small" else BIG()
    cases = [(1, CENTER, am.SEEDS[0]), (4, RANDOM, am.SEEDS[1])] if scene == "small" else [(3, RANDOM, am.SEEDS[0])]
    upload(gpu_ctx, spec)
    want = {c: am.aov(spec, *c) for c in cases}
    ran = set()
    for sc, tune, src_want in FAMILIES:
        if sc != scene:
            continue
        with tuning(gpu_ctx, **tune):
            for c in cases:
                got, st, src = render(gpu_ctx, capfd, spec, *c)
                assert src == src_want, (tune, src, src_want)
                same(got, want[c], (scene, tune, c))          # equal to the model, hence to each other
        ran.add(src_want)
    assert ran == ({22, 9, 7, 2, 8, 1, 0} if scene == "small" else {23, 5, 6, 8, 0, 2})


# ---- tile geometry -----------------------------------------------------------------------------

def test_tiles_and_bands_are_the_frames_pixels(gpu_ctx, capfd, specs):
    spec = specs["random"]                          # 64 x 48
    W, H = spec.width, spec.height
    upload(gpu_ctx, spec)
    for spp, jitter, seed in [(1, CENTER, 0), (4, RANDOM, am.SEEDS[0])]:
        frame, _, _ = render(gpu_ctx, capfd, spec, spp, jitter, seed)
        model = am.aov(spec, spp, jitter, seed)
        same(frame, model)
        # a tile with x0 and y0 above 0
        got, _, _ = render(gpu_ctx, capfd, spec, spp, jitter, seed, x0=5, tile_w=37, y0=7, tile_h=19)
        rows, cols = np.arange(7, 26), np.arange(5, 42)
        same(got, sub(frame, rows, cols), "tile")
        same(got, sub(model, rows, cols), "tile vs model")
        # a right-edge tile of width 1
        got, _, _ = render(gpu_ctx, capfd, spec, spp, jitter, seed, x0=W - 1, tile_w=1, y0=0, tile_h=H)
        same(got, sub(frame, np.arange(H), np.arange(W - 1, W)), "edge")
        # banded rows: band 2, stride 3, phase 1 from y0 = 3
        th = 14
        got, _, _ = render(gpu_ctx, capfd, spec, spp, jitter, seed, y0=3, tile_h=th, band=2, band_stride=3, band_phase=1)
        rows = np.array([3 + ((j // 2) * 3 + 1) * 2 + j % 2 for j in range(th)])
        assert rows.max() < H
        same(got, sub(frame, rows, np.arange(W)), "bands")
        same(got, sub(model, rows, np.arange(W)), "bands vs model")
    # an empty tile renders nothing and counts nothing
    arrays, st = gpu_ctx.render_aov(opts(spec, 2, CENTER, 0, tile_h=0))
    assert all(a.size == 0 for a in arrays.values())
    check_stats(st, 0, 2, CENTER)


# ---- channel masks -----------------------------------------------------------------------------

def test_only_the_selected_channels_are_written(gpu_ctx, capfd, specs):
    spec = specs["nan_plane"]                       # 17 x 13: odd sizes, NaN depths
    upload(gpu_ctx, spec)
    model = am.aov(spec, 4, RANDOM, am.SEEDS[1])
    masks = [BIT[n] for n in NAMES] + [lr.RT_AOV_DEPTH | lr.RT_AOV_OBJECT, lr.RT_AOV_NORMAL | lr.RT_AOV_COVERAGE]
    for mask in masks:
        out = {n: np.full_like(model[n], -12345) for n in NAMES}
        got, _, _ = render(gpu_ctx, capfd, spec, 4, RANDOM, am.SEEDS[1], channels=mask, out=out)
        for n in NAMES:
            if mask & BIT[n]:
                same({n: got[n]}, {n: model[n]}, (mask, n))
            else:
                assert (out[n] == -12345).all(), (mask, n, "written though not selected")
    # buffers of channels that are not selected may be absent altogether
    got, _, _ = render(gpu_ctx, capfd, spec, 4, RANDOM, am.SEEDS[1], channels=lr.RT_AOV_ALBEDO)
    assert set(got) == {"albedo"}
    same(got, {"albedo": model["albedo"]})


# ---- alignment with the beauty render ----------------------------------------------------------

@pytest.mark.parametrize("name", ["random", "inside"])
def test_albedo_lines_up_with_the_colours_of_the_flat_scene(gpu_ctx, capfd, specs, name):
    """Sample for sample: the flat scene (ambient = diffuse, nothing else) rendered by RT_ALGO_PATH and by
    RT_ALGO_WAVEFRONT_AA with random jitter and 4 samples is the original scene's albedo buffer."""
    spec = specs[name]
    seed = am.SEEDS[1]
    upload(gpu_ctx, spec)
    alb = render(gpu_ctx, capfd, spec, 4, RANDOM, seed, channels=lr.RT_AOV_ALBEDO)[0]["albedo"]
    upload(gpu_ctx, am.flat_albedo(spec, 4))
    for algo in (lr.RT_ALGO_PATH, lr.RT_ALGO_WAVEFRONT_AA):
        o = lr.render_opts(spec.width, spec.height, max_depth=2, spp=4, jitter=RANDOM, seed=seed, algo=algo,
                           flags=lr.RT_OUT_RGB_F32)
        rgb, _, _ = gpu_ctx.render(o, bgr=False)
        assert np.array_equal(am.bits(rgb), am.bits(alb)), (name, algo, int((am.bits(rgb) != am.bits(alb)).sum()))


# ---- lifecycle ---------------------------------------------------------------------------------

def test_aov_colour_aov_on_one_context(gpu_ctx, capfd, specs):
    spec = specs["random"]
    upload(gpu_ctx, spec)
    a, _, _ = render(gpu_ctx, capfd, spec, 3, CENTER, 0)
    o = lr.render_opts(spec.width, spec.height, max_depth=spec.max_depth, spp=1)
    rgb0, bgr0, st0 = gpu_ctx.render(o)
    b, _, _ = render(gpu_ctx, capfd, spec, 3, CENTER, 0)
    rgb1, bgr1, st1 = gpu_ctx.render(o)
    same(a, b)
    same(a, am.aov(spec, 3, CENTER, 0))
    assert np.array_equal(bgr0, bgr1) and np.array_equal(am.bits(rgb0), am.bits(rgb1))
    assert (st0.rays, st0.shadow_rays, st0.pixels) == (st1.rays, st1.shadow_rays, st1.pixels) and st0.chunks == st1.chunks


def test_statistics_read_late_and_kernel_time(gpu_ctx, specs):
    spec = specs["random"]
    px = spec.width * spec.height
    upload(gpu_ctx, spec)
    gpu_ctx.kernel_times()
    gpu_ctx.render_aov(opts(spec, 4, RANDOM, 3, flags=lr.RT_TIME_KERNELS), stats=False)
    gpu_ctx.render_aov(opts(spec, 2, CENTER, 3), lr.RT_AOV_DEPTH, stats=False)        # not timed
    for _ in range(2):                              # as often as wanted
        check_stats(gpu_ctx.stats(), px, 2, CENTER)
    kt = gpu_ctx.kernel_times()
    assert kt["camera"][1] == 1 and kt["camera"][0] > 0, kt
    assert sum(v[1] for v in kt.values()) == 1, kt
    upload(gpu_ctx, specs["tiny"])                  # another scene: the statistics stay the last render's
    check_stats(gpu_ctx.stats(), px, 2, CENTER)


def test_refusals_leave_the_statistics_alone(gpu_ctx, capfd, specs):
    spec = specs["random"]
    px = spec.width * spec.height
    upload(gpu_ctx, spec)
    render(gpu_ctx, capfd, spec, 3, CENTER, 0)

    def refused(code, o, channels=lr.RT_AOV_ALL, **kw):
        with pytest.raises(lr.RtError) as e:
            gpu_ctx.render_aov(o, channels, **kw)
        assert e.value.code == code, (e.value.code, code, str(e.value))
        check_stats(gpu_ctx.stats(), px, 3, CENTER)

    good = opts(spec, 1, CENTER, 0)
    refused(lr.RT_E_INVALID, good, 0)                                      # no channel
    refused(lr.RT_E_INVALID, good, 32)                                     # unknown bits
    refused(lr.RT_E_INVALID, good, lr.RT_AOV_ALL | 64)
    refused(lr.RT_E_INVALID, good, lr.RT_AOV_DEPTH, out={})                # a selected channel's pointer is NULL
    refused(lr.RT_E_INVALID, good, lr.RT_AOV_ALL, out={n: np.zeros((spec.height, spec.width, 3), np.float32)
                                                      for n in ("normal", "albedo")})
    refused(lr.RT_E_INVALID, opts(spec, 1, CENTER, 0, x0=1))               # geometry rt_render refuses
    refused(lr.RT_E_INVALID, opts(spec, 1, CENTER, 0, y0=1))
    refused(lr.RT_E_INVALID, opts(spec, 1, CENTER, 0, band_stride=2, band_phase=2))
    refused(lr.RT_E_INVALID, opts(spec, 1, 2, 0))                          # jitter mode
    o = opts(spec, 1, CENTER, 0)
    o.width = 0
    refused(lr.RT_E_INVALID, o)
    # the device entry point refuses the same way
    with pytest.raises(lr.RtError) as e:
        gpu_ctx.render_aov_device(good, lr.RT_AOV_DEPTH, {"depth": 0})
    assert e.value.code == lr.RT_E_INVALID
    with pytest.raises(lr.RtError) as e:
        gpu_ctx.render_aov_device(good, 0, {})
    assert e.value.code == lr.RT_E_INVALID
    check_stats(gpu_ctx.stats(), px, 3, CENTER)
    # a DepthOfField camera: refused, and the previous render's statistics stay
    dof = scenes.stochastic(width=48, height=32, dof=True)
    upload(gpu_ctx, dof)
    with pytest.raises(lr.RtError) as e:
        gpu_ctx.render_aov(opts(dof, 1, RANDOM, 0))
    assert e.value.code == lr.RT_E_UNSUPPORTED and "DepthOfField" in str(e.value)
    check_stats(gpu_ctx.stats(), px, 3, CENTER)
    # no scene uploaded
    with lr.Context(0) as fresh:
        with pytest.raises(lr.RtError) as e:
            fresh.render_aov(good)
        assert e.value.code == lr.RT_E_NOSCENE
        with pytest.raises(lr.RtError) as e:
            fresh.render_aov(good, 0)
        assert e.value.code == lr.RT_E_INVALID


# ---- rt_render_aov_device on a torch stream ----------------------------------------------------

_DEVICE = r"""
import sys
sys.path[:0] = sys.argv[1:4]
import numpy as np
import torch                      # first: the process then uses torch's HIP runtime for both
import libraytrace as lr
from libraytrace import scenes

spec = scenes.random_spheres(64, 64, 48, 4, seed=9, plane=True, name="aov_rand")
W, H = spec.width, spec.height
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(dev)               # not torch's default stream
assert stream.cuda_stream != 0
X0, Y0, TW, TH = 3, 5, 50, 31
SENT = -777.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


with lr.Context(0) as ctx:
    ctx.upload(lr.Scene.deserialize(spec.to_text()))
    for spp, jitter, mask in ((3, 0, 31), (4, 1, 31), (4, 1, lr.RT_AOV_NORMAL | lr.RT_AOV_OBJECT)):
        o = lr.render_opts(W, H, spp=spp, jitter=jitter, seed=11, x0=X0, tile_w=TW, y0=Y0, tile_h=TH)
        host, st_host = ctx.render_aov(o, mask)
        t = {"depth": torch.full((TH, TW), SENT, dtype=torch.float32, device=dev),
             "normal": torch.full((TH, TW, 3), SENT, dtype=torch.float32, device=dev),
             "albedo": torch.full((TH, TW, 3), SENT, dtype=torch.float32, device=dev),
             "coverage": torch.full((TH, TW), SENT, dtype=torch.float32, device=dev),
             "object": torch.full((TH, TW), -777, dtype=torch.int32, device=dev)}
        colour = torch.zeros((H, 3 * W), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        # a colour render between the two, on the context's own stream: the AOV render is ordered after it
        ctx.render_device(lr.render_opts(W, H, max_depth=4, spp=1, flags=lr.RT_OUT_BGR_U8), 0, colour.data_ptr())
        ctx.render_aov_device(o, mask, {k: v.data_ptr() for k, v in t.items()}, stream.cuda_stream)
        st = ctx.stats()                      # synchronises with the render
        stream.synchronize()
        assert (st.rays, st.shadow_rays, st.pixels, st.traced_rays, st.chunks) == \
               (st_host.rays, 0, TW * TH, st_host.traced_rays, 0), (st.rays, st.pixels, st.traced_rays)
        assert st.rays == TW * TH * spp
        for name, bit in (("depth", 1), ("normal", 2), ("albedo", 4), ("coverage", 8), ("object", 16)):
            got = t[name].cpu().numpy()
            if mask & bit:
                assert np.array_equal(bits(got), bits(host[name])), (name, spp, jitter)
            else:
                assert (got == SENT).all(), (name, "written though not selected")
print("aov_device ok")
"""


def test_device_buffers_on_a_torch_stream():
    """rt_render_aov_device into torch device buffers on a non-default stream equals the host variant, bit for
    bit; unselected buffers keep their sentinel.  In a child process: torch must initialise HIP before the
    library does."""
    out = subprocess.run([sys.executable, "-c", _DEVICE, ROOT, os.path.join(ROOT, "rust-raytrace_amd"),
                          os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "aov_device ok" in out.stdout, out.stderr[-3000:]


# ---- the CLI -----------------------------------------------------------------------------------

def read_pfm(path):
    data = open(path, "rb").read()
    head = data.split(b"\n", 3)
    kind, (w, h), scale = head[0], [int(x) for x in head[1].split()], float(head[2])
    assert kind in (b"PF", b"Pf") and scale < 0           # little-endian
    ch = 3 if kind == b"PF" else 1
    a = np.frombuffer(head[3], "<f4")
    assert a.size == w * h * ch, (path, a.size, w, h, ch)
    return a.reshape((h, w, 3) if ch == 3 else (h, w))


def test_cli_writes_the_five_buffers(gpu_ctx, capfd, specs, tmp_path):
    spec = specs["random"]
    scene = tmp_path / "scene.txt"
    scene.write_text(spec.to_text())
    prefix = str(tmp_path / "out")
    run = subprocess.run([EXE, "--scene", str(scene), "--aov", prefix, "--spp", "4", "--jitter", "random", "--seed", "7"],
                         capture_output=True, text=True, timeout=100)
    assert run.returncode == 0, run.stdout + run.stderr
    upload(gpu_ctx, spec)
    want, _, _ = render(gpu_ctx, capfd, spec, 4, RANDOM, 7)
    for n in FLOATS:
        got = read_pfm(f"{prefix}.{n}.pfm")
        assert got.shape == want[n].shape
        assert got.tobytes() == want[n].tobytes(), n          # bottom-up rows: the library's row order
    ids = read_pfm(f"{prefix}.object.pfm")
    assert np.array_equal(ids, want["object"].astype(np.float32))
    assert not os.path.exists(str(tmp_path / "out.bmp"))
    # more than one device is out of scope: refused with a message
    run = subprocess.run([EXE, "--scene", str(scene), "--aov", prefix, "--gpus", "2"], capture_output=True, text=True,
                         timeout=100)
    assert run.returncode == 2 and "--aov" in run.stdout, run.stdout + run.stderr
