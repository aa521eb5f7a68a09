"""The statistics of a render, read late: after other calls on the same context.

Every other GPU test reads a render's statistics in the call that rendered it.  The
hot path does not: rt_render without an rt_stats and rt_render_device leave the
tally of a one-chunk wavefront render pending (rt_ctx.hpp PendingTally, pointers
into the lane's working set) until rt_ctx_stats / rt_ctx_generation_counts ask.
Here something else happens in between -- a reserve that grows or keeps the
working set, a retune that rebuilds the lanes, another scene, a refused call,
another render -- and the counts read afterwards must still be that render's.

What is asserted comes from the oracle (ref64) or from identities on its counts;
the per-generation queue sizes, which the oracle does not report, are compared with
those of a fresh context that renders and reads at once (and RT_COUNT_WORK's test
counts, which depend on the tree walk, with an undisturbed counted render).  A case
that aims at a release of the working set proves it from the library's verbose
line `rtamd: lane working set released (N MB), tally settled 1`.

Every case has its own context: the working set must be exactly what the first
render allocated, and a case that goes wrong must not take other tests with it.

Not run here: the RT_E_NOMEM retry (ensure_wavefront) frees working sets too, but
only frames far beyond a few seconds reach it
(test_oversized_budget_falls_back_to_smaller_chunks).  It frees through the same
release_lane_memory as every case below, and the settling of a pending tally
lives in that function, so it is covered by construction.

The last test drives rt_render_device (device buffers, a caller's stream) against
the oracle for every schedule: tile offsets, a padded BGR pitch whose padding is
the caller's, f32, and the counts read after the asynchronous call.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libraytrace as lr
from libraytrace import scenes
from oracle import ref64
from test_gpu_parity import check_close

pytestmark = pytest.mark.gpu

W, H, DEPTH = 64, 48, 8
N_LIGHTS = 2                                   # config3's and config2's point lights
RELEASE = re.compile(r"rtamd: lane working set released \((\d+) MB\), tally settled (\d)")
ONE_CHUNK = re.compile(r"rtamd: chunks 1 x \d+ rows \(first \d+\), lanes 1,")
COUNTED = lr.RT_OUT_RGB_F32 | lr.RT_OUT_BGR_U8 | lr.RT_COUNT_WORK


def r1_opts(**kw):
    kw = dict(dict(max_depth=DEPTH, spp=1, algo=lr.RT_ALGO_WAVEFRONT), **kw)
    return lr.render_opts(W, H, **kw)


def big_opts():
    return lr.render_opts(512, 384, max_depth=DEPTH, spp=1, algo=lr.RT_ALGO_WAVEFRONT)


def three_lights():
    spec = scenes.config2(40, 24)
    spec.directional_light((0.2, -1.0, -0.3), (0.2, 0.2, 0.2))
    assert len(spec.lights) != N_LIGHTS
    return spec


_cache = {}


def refs():
    """Computed once and left unchanged: the oracle's renders, and what a fresh
    context reports for R1 when it reads at once."""
    if not _cache:
        r1, c2 = scenes.config3(W, H), scenes.config2(40, 24)
        assert len(r1.lights) == N_LIGHTS and len(c2.lights) == N_LIGHTS and r1.max_depth == DEPTH
        _cache["r1_text"], _cache["c2_text"] = r1.to_text(), c2.to_text()
        _cache["r1"] = ref64.render(r1)
        _cache["r1_d4"] = ref64.render(r1, max_depth=4)
        _cache["c2"] = ref64.render(c2)
        with lr.Context(0) as ctx:
            ctx.upload(lr.Scene.deserialize(_cache["r1_text"]))
            _, _, st = ctx.render(r1_opts())
            assert st.rays == _cache["r1"]["counts"]["rays"]
            _cache["qs"] = ctx.generation_counts()
            _cache["counted"] = ctx.render(r1_opts(flags=COUNTED))[2]
    return _cache


@pytest.fixture
def ctx():
    if lr.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need an MI355X (no CPU fallback exists)")
    c = lr.Context(0, tuning={"verbose": 1})
    yield c
    c.close()


def render_r1_lazy(ctx, capfd, **kw):
    """R1 through rt_render without an rt_stats: one chunk on one lane (by the verbose
    line), so its tally is left pending.  -> (rgb, bgr)"""
    ctx.upload(lr.Scene.deserialize(refs()["r1_text"]))
    capfd.readouterr()
    rgb, bgr, st = ctx.render(r1_opts(**kw), stats=False)
    assert st is None
    assert ONE_CHUNK.search(capfd.readouterr().err)
    return rgb, bgr


def assert_counts(st, ref, pixels):
    assert (st.rays, st.shadow_rays, st.pixels) == (ref["counts"]["rays"], ref["counts"]["shadow_rays"], pixels)


def assert_r1_read(ctx):
    """rt_ctx_stats and rt_ctx_generation_counts report R1: the oracle's counts, the
    identities between the per-generation sizes and them, a fresh context's sizes."""
    r = refs()
    cnt = r["r1"]["counts"]
    st = ctx.stats()
    assert_counts(st, r["r1"], W * H)
    q, s = ctx.generation_counts()
    assert sum(q[1:]) + W * H == cnt["rays"] - cnt["shadow_rays"]
    assert sum(s) * N_LIGHTS == cnt["shadow_rays"]
    assert (q, s) == r["qs"]
    return st


def assert_context_still_renders(ctx, first):
    """After the read: another scene against the oracle (bytes, f32, counts), then R1
    again, bit for bit the first R1."""
    r = refs()
    ctx.upload(lr.Scene.deserialize(r["c2_text"]))
    rgb, bgr, st = ctx.render(lr.render_opts(40, 24, max_depth=4, spp=1))
    assert np.array_equal(bgr, r["c2"]["bgr"])
    check_close(rgb, r["c2"]["rgb64"])
    assert_counts(st, r["c2"], 40 * 24)
    ctx.upload(lr.Scene.deserialize(r["r1_text"]))
    rgb, bgr, st = ctx.render(r1_opts())
    assert np.array_equal(bgr, first[1]) and np.array_equal(rgb.view(np.uint32), first[0].view(np.uint32))
    assert_counts(st, r["r1"], W * H)


def _refused(call):
    with pytest.raises(lr.RtError) as e:
        call()
    assert e.value.code == lr.RT_E_INVALID


def _multi_lane_reserve(ctx):
    ctx.set_tuning("chunk_pixels", 64 * 8)
    ctx.set_tuning("lanes", 2)
    ctx.reserve(r1_opts())


# (the call between R1 and the read, does the working set go: True / False / None = not asserted)
BETWEEN = [
    pytest.param(lambda ctx: None, False, id="nothing"),
    pytest.param(lambda ctx: ctx.reserve(r1_opts()), False, id="reserve_same"),
    pytest.param(lambda ctx: ctx.reserve(big_opts(), host=False), True, id="reserve_larger_tile_device"),
    pytest.param(lambda ctx: ctx.reserve(big_opts(), host=True), True, id="reserve_larger_tile_host"),
    pytest.param(lambda ctx: ctx.reserve(r1_opts(max_depth=30)), True, id="reserve_deeper"),
    pytest.param(lambda ctx: ctx.set_tuning("prio", 0), True, id="retune_prio"),
    pytest.param(lambda ctx: ctx.set_tuning("cu_mask", 0), True, id="retune_cu_mask"),
    pytest.param(lambda ctx: ctx.set_tuning("a_queue", 1), True, id="retune_a_queue"),
    pytest.param(lambda ctx: ctx.set_tuning("prio", 1), False, id="retune_same_value"),
    pytest.param(lambda ctx: ctx.upload(lr.Scene.deserialize(three_lights().to_text())), False, id="upload_other_scene"),
    pytest.param(lambda ctx: _refused(lambda: ctx.render(r1_opts(x0=40, tile_w=40))), False, id="refused_render"),
    pytest.param(lambda ctx: _refused(lambda: ctx.reserve(r1_opts(y0=20, tile_h=40))), False, id="refused_reserve"),
    pytest.param(_multi_lane_reserve, None, id="reserve_two_lanes"),
]


@pytest.mark.parametrize("between,released", BETWEEN)
def test_pending_statistics_survive(ctx, capfd, between, released):
    assert ctx.get_tuning("prio") == 1 and ctx.get_tuning("cu_mask") != 0 and ctx.get_tuning("a_queue") == 0
    first = render_r1_lazy(ctx, capfd)
    assert np.array_equal(first[1], refs()["r1"]["bgr"])
    between(ctx)
    lines = RELEASE.findall(capfd.readouterr().err)
    if released is True:
        assert lines and lines[0][1] == "1", lines        # the path aimed at was taken, and it settled the tally
        assert all(settled == "0" for _, settled in lines[1:]), lines
    elif released is False:
        assert not lines, lines
    st = assert_r1_read(ctx)
    again = ctx.stats()
    assert (again.rays, again.shadow_rays, again.pixels, again.chunks) == (st.rays, st.shadow_rays, st.pixels, st.chunks)
    assert ctx.generation_counts() == refs()["qs"]
    assert not RELEASE.findall(capfd.readouterr().err)    # reading releases nothing
    assert_context_still_renders(ctx, first)


# ---- sequences whose counters could leak from one render into the next ----

def test_brute_render_after_a_pending_tally(ctx, capfd):
    render_r1_lazy(ctx, capfd)
    _, _, st = ctx.render(r1_opts(max_depth=4, algo=lr.RT_ALGO_BRUTE_LDS))
    assert_counts(st, refs()["r1_d4"], W * H)
    assert_counts(ctx.stats(), refs()["r1_d4"], W * H)


def test_pending_tally_after_an_unread_brute_render(ctx, capfd):
    """The megakernel's per-shard counters are still set when the lazy render ends: the
    flush clears them before its tally."""
    ctx.upload(lr.Scene.deserialize(refs()["r1_text"]))
    ctx.render(r1_opts(max_depth=4, algo=lr.RT_ALGO_BRUTE_LDS), stats=False)
    render_r1_lazy(ctx, capfd)
    assert_r1_read(ctx)


def test_counted_render_settled_by_a_growing_reserve(ctx, capfd):
    """RT_COUNT_WORK: the render's own test counts are in the counters already, and the
    settled tally adds the ray counts to them."""
    render_r1_lazy(ctx, capfd, flags=COUNTED)
    ctx.reserve(big_opts())
    lines = RELEASE.findall(capfd.readouterr().err)
    assert lines and lines[0][1] == "1", lines
    st = assert_r1_read(ctx)
    want = refs()["counted"]
    assert st.box_tests > 0 and st.sphere_tests > 0
    assert (st.box_tests, st.sphere_tests, st.shadow_box_tests, st.shadow_sphere_tests) == \
           (want.box_tests, want.sphere_tests, want.shadow_box_tests, want.shadow_sphere_tests)


def test_pending_tally_after_an_unread_multi_chunk_render(ctx, capfd):
    """Three chunks tally eagerly into the counters; the one-chunk render after them
    must not add to that."""
    ctx.upload(lr.Scene.deserialize(refs()["r1_text"]))
    ctx.set_tuning("chunk_pixels", 64 * 16)
    capfd.readouterr()
    ctx.render(r1_opts(), stats=False)
    assert re.search(r"rtamd: chunks 3 x 16 rows", capfd.readouterr().err)
    ctx.set_tuning("chunk_pixels", 0)
    render_r1_lazy(ctx, capfd)
    st = assert_r1_read(ctx)
    assert st.chunks == 1


def test_empty_tile_after_a_pending_tally(ctx, capfd):
    render_r1_lazy(ctx, capfd)
    ctx.render(r1_opts(tile_h=0), stats=False)
    st = ctx.stats()
    assert (st.rays, st.shadow_rays, st.pixels) == (0, 0, 0)


def test_path_render_after_a_pending_tally(ctx, capfd):
    render_r1_lazy(ctx, capfd)
    ctx.upload(lr.Scene.deserialize(refs()["c2_text"]))
    _, bgr, _ = ctx.render(lr.render_opts(40, 24, max_depth=4, spp=1, algo=lr.RT_ALGO_PATH), stats=False)
    assert np.array_equal(bgr, refs()["c2"]["bgr"])
    assert_counts(ctx.stats(), refs()["c2"], 40 * 24)


# ---- rt_render_device against the oracle ----

_RENDER_DEVICE = r"""
import sys
sys.path[:0] = sys.argv[1:4]
import numpy as np
import torch                      # first: the process then uses torch's HIP runtime for both
import libraytrace as lr
from libraytrace import scenes
from oracle import ref64
from test_gpu_parity import check_close

W, H, DEPTH = 64, 48, 8
X0, Y0, TW, TH = 8, 5, 40, 30
PITCH, GUARD = 3 * TW + 5, 256
spec = scenes.config3(W, H)                   # Phong only: the path kernel is bit-exact on it too
tile = dict(x0=X0, tile_w=TW, y0=Y0, tile_h=TH)
ref_tile = ref64.render(spec, max_depth=DEPTH, **tile)
ref_d3 = ref64.render(spec, max_depth=3)
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(dev)               # not torch's default stream
assert stream.cuda_stream != 0


def counts(st, ref, pixels):
    assert (st.rays, st.shadow_rays, st.pixels) == (ref["counts"]["rays"], ref["counts"]["shadow_rays"], pixels), \
        (st.rays, st.shadow_rays, st.pixels, ref["counts"])


def buffers(rows, cols, pitch):
    # guard bytes before and after the BGR rows; f32 starts as NaN
    raw = torch.full((GUARD + rows * pitch + GUARD,), 0xCD, dtype=torch.uint8, device=dev)
    rgb = torch.full((rows, cols, 3), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    return raw, rgb


def tile_opts(algo, **kw):
    return lr.render_opts(W, H, max_depth=DEPTH, spp=1, algo=algo, bgr_pitch=PITCH, **dict(tile, **kw))


with lr.Context(0, tuning={"verbose": 1}) as ctx:
    ctx.upload(lr.Scene.deserialize(spec.to_text()))
    for algo in (lr.RT_ALGO_WAVEFRONT, lr.RT_ALGO_WAVEFRONT_BRUTE, lr.RT_ALGO_BRUTE_LDS, lr.RT_ALGO_BRUTE_GLOBAL,
                 lr.RT_ALGO_PATH):
        raw, rgb = buffers(TH, TW, PITCH)
        ctx.render_device(tile_opts(algo), rgb.data_ptr(), raw.data_ptr() + GUARD, stream.cuda_stream)
        st = ctx.stats()                      # synchronises with the render
        stream.synchronize()
        got = raw.cpu().numpy()
        rows = got[GUARD:GUARD + TH * PITCH].reshape(TH, PITCH)
        assert np.array_equal(rows[:, :3 * TW], ref_tile["bgr"]), (algo, int((rows[:, :3 * TW] != ref_tile["bgr"]).sum()))
        assert (rows[:, 3 * TW:] == 0xCD).all(), (algo, "row padding written")
        assert (got[:GUARD] == 0xCD).all() and (got[GUARD + TH * PITCH:] == 0xCD).all(), (algo, "guard bytes written")
        check_close(rgb.cpu().numpy(), ref_tile["rgb64"])
        counts(st, ref_tile, TW * TH)

    # two renders with different options, nothing between them: the statistics are the second's
    raw, rgb = buffers(TH, TW, PITCH)
    raw2, rgb2 = buffers(H, W, 3 * W)
    ctx.render_device(tile_opts(lr.RT_ALGO_WAVEFRONT), rgb.data_ptr(), raw.data_ptr() + GUARD, stream.cuda_stream)
    ctx.render_device(lr.render_opts(W, H, max_depth=3, spp=1, algo=lr.RT_ALGO_WAVEFRONT), rgb2.data_ptr(),
                      raw2.data_ptr() + GUARD, stream.cuda_stream)
    counts(ctx.stats(), ref_d3, W * H)
    stream.synchronize()
    assert np.array_equal(raw2.cpu().numpy()[GUARD:GUARD + H * 3 * W].reshape(H, 3 * W), ref_d3["bgr"])
    assert np.array_equal(raw.cpu().numpy()[GUARD:GUARD + TH * PITCH].reshape(TH, PITCH)[:, :3 * TW], ref_tile["bgr"])
    check_close(rgb2.cpu().numpy(), ref_d3["rgb64"])

    # a lazy render, then a reserve that frees its working set, then the read: the render's counts
    raw, rgb = buffers(TH, TW, PITCH)
    ctx.render_device(tile_opts(lr.RT_ALGO_WAVEFRONT), rgb.data_ptr(), raw.data_ptr() + GUARD, stream.cuda_stream)
    print("before reserve", file=sys.stderr, flush=True)
    ctx.reserve(lr.render_opts(512, 384, max_depth=DEPTH, spp=1, algo=lr.RT_ALGO_WAVEFRONT), host=False,
                stream_ptr=stream.cuda_stream)
    print("after reserve", file=sys.stderr, flush=True)
    counts(ctx.stats(), ref_tile, TW * TH)
    counts(ctx.stats(), ref_tile, TW * TH)
    stream.synchronize()
    assert np.array_equal(raw.cpu().numpy()[GUARD:GUARD + TH * PITCH].reshape(TH, PITCH)[:, :3 * TW], ref_tile["bgr"])
print("render_device ok")
"""


def test_render_device_matches_oracle():
    """rt_render_device on a torch stream, every schedule: a tile at an offset into a
    padded, 0xCD-filled BGR buffer (pixels the oracle's, padding and guard bytes
    untouched), f32 within RTOL, counts read after the asynchronous call; two renders
    back to back; a render whose working set a reserve frees before the read.
    In a child process: torch must initialise HIP before the library does."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _RENDER_DEVICE, root, os.path.join(root, "rust-raytrace_amd"),
                          os.path.join(root, "tests")], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "render_device ok" in out.stdout, out.stderr[-3000:]
    during = out.stderr.split("before reserve")[1].split("after reserve")[0]
    lines = RELEASE.findall(during)
    assert lines and lines[0][1] == "1", out.stderr[-3000:]
