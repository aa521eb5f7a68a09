"""The output stage on the device, bit for bit ("Output stage").

Part one: rt_accum_upload + rt_accum_resolve run accum_resolve on operands of the caller's choice: every
sRGB threshold, the values either side of it, the f32 rounding's ties, denormals and overflow, as quotients
sum / n for n in 1, 2, 3, 7, 1000 and 2^31.  The f32 output must be to_f32(sum / n) and the bytes
quantise(sum / n) (output_model.py: quantised from the f64 value), through byte stores, dword stores and
the host resolve.

Part two: the threshold scenes (threshold_scenes.py) make every threshold and its lower neighbour the exact
f64 colour of some pixels by three routes, and every schedule that writes pixels must then write the
oracle's bytes, the oracle's f32 bits and trace the oracle's rays.  WRITERS names, for each of the nine
copies of the sRGB table on the device, the cases whose threshold pixels are quantised through that copy.

The oracle's renders are computed once per (route, spp, jitter) and left unchanged.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import libraytrace as lr
from oracle import ref64

import output_model as om
import threshold_scenes as ts

pytestmark = pytest.mark.gpu

SEED = 7
MEGA_LDS, MEGA_GLOBAL, WF, WF_BRUTE = lr.RT_ALGO_BRUTE_LDS, lr.RT_ALGO_BRUTE_GLOBAL, lr.RT_ALGO_WAVEFRONT, lr.RT_ALGO_WAVEFRONT_BRUTE
PATH, AA = lr.RT_ALGO_PATH, lr.RT_ALGO_WAVEFRONT_AA


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


# ---- part one: accum_resolve as an operand probe ------------------------------------------------------

TILE_W = 197                                   # no multiple of 64: every row ends in a partial segment
PITCH_DWORDS = 3 * TILE_W + 9                  # 600: a multiple of 4 with slack (dword stores); 0 -> 591: byte stores


def _hip():
    hip = lr.lib          # the HIP runtime librtamd.so is linked against (test_gpu_aa.py)
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    return hip


def _resolve_device(ctx, acc, pitch):
    """rt_accum_resolve into device buffers with guard bytes around the rows -> (rgb, bgr rows [h, pitch])."""
    hip, guard = _hip(), 256
    p = pitch or 3 * acc.tile_w
    n_bgr = guard + acc.tile_h * p + guard
    h_bgr = np.full(n_bgr, 0xCD, np.uint8)
    h_rgb = np.full((acc.tile_h, acc.tile_w, 3), np.nan, np.float32)
    d_bgr, d_rgb = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d_bgr), n_bgr) == 0 and hip.hipMalloc(ctypes.byref(d_rgb), h_rgb.nbytes) == 0
    try:
        assert hip.hipMemcpy(d_bgr, h_bgr.ctypes.data, n_bgr, 1) == 0
        assert hip.hipMemcpy(d_rgb, h_rgb.ctypes.data, h_rgb.nbytes, 1) == 0
        acc.resolve_device(d_rgb.value, d_bgr.value + guard, pitch=pitch)
        ctx.stats()                            # synchronises with the context's stream
        assert hip.hipMemcpy(h_bgr.ctypes.data, d_bgr, n_bgr, 2) == 0
        assert hip.hipMemcpy(h_rgb.ctypes.data, d_rgb, h_rgb.nbytes, 2) == 0
    finally:
        hip.hipFree(d_bgr)
        hip.hipFree(d_rgb)
    assert (h_bgr[:guard] == 0xCD).all() and (h_bgr[-guard:] == 0xCD).all(), "guard bytes written"
    return h_rgb, h_bgr[guard:-guard].reshape(acc.tile_h, p)


@pytest.fixture(scope="module")
def probe_scene(gpu_ctx):
    """Any small scene: an accumulator binds to the uploaded scene, the resolve never reads it."""
    gpu_ctx.upload(lr.Scene.deserialize(ts.background_scenes()[0].to_text()))
    return gpu_ctx


def _report(what, n, bad, sums, tile_shape, got, want):
    k = np.flatnonzero(bad.reshape(-1))
    flat = np.zeros(int(np.prod(tile_shape)))
    flat[:sums.size] = sums
    first = [(float(flat[i]).hex(), got.reshape(-1)[i], want.reshape(-1)[i]) for i in k[:4]]
    return f"n = {n}, {what}: {k.size} of {bad.size} records differ; first (sum, device, model): {first}"


@pytest.mark.parametrize("n", om.SAMPLES, ids=lambda n: f"n{n}")
def test_accum_resolve_is_the_model_bit_for_bit(probe_scene, n):
    """Every record through rt_accum_resolve_host with byte stores and with dword stores (padding zero) and
    through rt_accum_resolve (padding and guard bytes untouched): f32 = to_f32(sum / n), bytes =
    quantise(sum / n), NaN by position.  The coverage conditions are asserted first, from the model."""
    ctx = probe_scene
    sums, _, _ = om.probe_sums(n)
    cov = om.threshold_coverage(sums, n)
    assert cov.all(), np.argwhere(~cov)[:5]
    q = om.average(sums, n)
    cls = om.f32_class(q)
    for name in om.CLASSES:
        assert cls[name].sum() >= 100, (name, int(cls[name].sum()))
    tile, used = om.probe_tile(sums, TILE_W)
    rows = tile.shape[0]
    want64 = om.average(tile, n)
    want32 = om.to_f32(want64)
    want_bgr = om.bgr_rows(want64)
    ends = want_bgr.reshape(rows, TILE_W, 3)[:, -1, :]
    print(f"n = {n}: {used} records in {rows} rows of {TILE_W}; classes "
          + ", ".join(f"{k} {int(cls[k].sum())}" for k in om.CLASSES)
          + f"; {len(np.unique(ends))} byte values at the row ends")
    with ctx.accumulator(lr.render_opts(TILE_W, rows, spp=1)) as acc:
        acc.upload(tile, n)
        assert acc.samples == n
        for how, pitch in (("host bytes", 0), ("host dwords", PITCH_DWORDS), ("device bytes", 0), ("device pitched", PITCH_DWORDS)):
            if how.startswith("host"):
                rgb, bgr = acc.resolve(pitch=pitch)
                assert (bgr[:, 3 * TILE_W:] == 0).all(), f"{how}: padding not zero"
            else:
                rgb, bgr = _resolve_device(ctx, acc, pitch)
                assert (bgr[:, 3 * TILE_W:] == 0xCD).all(), f"{how}: padding written"
            bad32 = ~om.same_f32(rgb, want32)
            assert not bad32.any(), _report(how + " f32", n, bad32, sums, tile.shape, rgb, want32)
            got = bgr[:, :3 * TILE_W].reshape(rows, TILE_W, 3)[:, :, ::-1]
            bad8 = got != want_bgr.reshape(rows, TILE_W, 3)[:, :, ::-1]
            assert not bad8.any(), _report(how + " bytes", n, bad8, sums, tile.shape, got, om.quantise(want64))
        back, samples = acc.download()
        assert samples == n and np.array_equal(back.view(np.uint64), tile.view(np.uint64))       # resolve reads only


def test_row_ends_see_every_byte_value(probe_scene):
    """The store path's masks at the row ends: a tile whose last pixels of the rows run through all 256 byte
    values in each channel position, 1 .. 5, 64, 65 and 197 pixels wide, both layouts of both resolves (a
    device resolve takes the dword path only where 3 * width is a multiple of 4: widths 4 and 64)."""
    ctx = probe_scene
    t = om.TABLE
    val = np.concatenate([[0.0], t])           # val[k] quantises to k
    assert om.quantise(val).tolist() == list(range(256))
    for w in (TILE_W, 1, 2, 3, 4, 5, 64, 65):
        tile = np.full((256, w, 3), 0.25)
        tile[:, -1, 0] = val
        tile[:, -1, 1] = val[::-1]
        tile[:, -1, 2] = np.roll(val, 85)
        tile[:, 0, 2] = np.roll(val, 170)
        want = om.bgr_rows(tile)
        with ctx.accumulator(lr.render_opts(w, 256, spp=1)) as acc:
            acc.upload(tile * 2.0, 2)
            for pitch in (0, (3 * w + 3) // 4 * 4 + 4):
                rgb, bgr = acc.resolve(pitch=pitch)
                assert np.array_equal(bgr[:, :3 * w], want), (w, pitch)
                assert (bgr[:, 3 * w:] == 0).all(), (w, pitch)
                assert om.same_f32(rgb, om.to_f32(tile)).all(), (w, pitch)
                _, dbgr = _resolve_device(ctx, acc, pitch)
                assert np.array_equal(dbgr[:, :3 * w], want) and (dbgr[:, 3 * w:] == 0xCD).all(), (w, pitch)


# ---- part two: the threshold scenes -------------------------------------------------------------------

_refs = {}


def oracle(route, spp=1, jitter=0):
    k = (route, spp, jitter)
    if k not in _refs:
        r = ref64.render(ts.scene(route, spp), jitter=jitter, seed=SEED, rng=1 if jitter else 0)
        # the coverage condition, before any comparison: every one of the 510 values, exactly, on this route
        assert ts.values_present(r["rgb64"]).all() and ts.pixels_per_triple(r["rgb64"]).min() >= 64, k
        assert om.same_f32(om.to_f32(r["rgb64"]), r["rgb32"]).all() and np.array_equal(om.bgr_rows(r["rgb64"]), r["bgr"])
        _refs[k] = r
    return _refs[k]


def _case(name, algo, tune=None, spp=1, jitter=0, accum=False):
    return dict(name=name, algo=algo, tune=tune or {}, spp=spp, jitter=jitter, accum=accum)


OFF_GRID = dict(cam_grid_res=-1, light_grids=0)     # the camera pass per ray through `src`, shadows through src_occ
CASES = [
    _case("mega_lds", MEGA_LDS), _case("mega_global", MEGA_GLOBAL), _case("wavefront", WF), _case("wavefront_brute", WF_BRUTE),
    _case("path", PATH),
    _case("compose0", WF, dict(compose=0)), _case("compose1", WF, dict(compose=1)),
    _case("tail0", WF, dict(tail_fuse=0)), _case("tail1", WF, dict(tail_fuse=1)), _case("tail2", WF, dict(tail_fuse=2)),
    _case("tail1_compose1", WF, dict(tail_fuse=1, compose=1)),
    _case("src9_bvh", WF, dict(OFF_GRID, src=9, src_occ=10)), _case("src7_bvh", WF, dict(OFF_GRID, src=7, src_occ=7)),
    _case("src8_prefix", WF, dict(OFF_GRID, src=8, src_occ=11, prefix_kb=1)),
    _case("src25_q4", WF, dict(OFF_GRID, src=25, src_occ=11)),
    _case("src26_q4", WF, dict(OFF_GRID, src=26, src_occ=11, prefix_kb=1)),
    _case("src8_compose1", WF, dict(OFF_GRID, src=8, src_occ=11, prefix_kb=1, compose=1)),
    _case("spp2_centre_wavefront", WF, spp=2), _case("spp2_centre_compose1", WF, dict(compose=1), spp=2),
    _case("spp2_centre_mega_lds", MEGA_LDS, spp=2), _case("spp2_centre_path", PATH, spp=2),
    _case("spp2_random_path", PATH, spp=2, jitter=1),
    _case("spp2_random_aa_compose0", AA, dict(compose=0), spp=2, jitter=1),
    _case("spp2_random_aa_compose1", AA, dict(compose=1), spp=2, jitter=1),
    _case("accum_1+1_path", PATH, spp=2, jitter=1, accum=True),
    _case("accum_1+1_aa_compose0", AA, dict(compose=0), spp=2, jitter=1, accum=True),
    _case("accum_1+1_aa_compose1", AA, dict(compose=1), spp=2, jitter=1, accum=True),
]
CASE_NAMES = [c["name"] for c in CASES]

# The nine copies of the sRGB table on the device, and the cases (route-case) whose THRESHOLD pixels are
# quantised through each: shown to be true by leaving each copy unfilled in turn (the
# mutation table: exactly these cases fail).  Route A's pixels are written by whatever finishes the camera
# pass; B's and C's by the fold or the fused tail, also under compose (emit_chain packs the bytes, wf_compose
# copies them); random jitter and the accumulators end in accum_resolve (wf_output).
_WF_A = ("wavefront", "wavefront_brute", "compose0", "tail0", "tail1", "tail2", "spp2_centre_wavefront")
_FOLD = ("wavefront", "wavefront_brute", "compose0", "compose1", "tail0", "tail2", "src9_bvh", "src7_bvh", "src8_prefix",
         "src25_q4", "src26_q4", "src8_compose1", "spp2_centre_wavefront", "spp2_centre_compose1")
_RESOLVE = ("spp2_random_aa_compose0", "spp2_random_aa_compose1", "accum_1+1_path", "accum_1+1_aa_compose0",
            "accum_1+1_aa_compose1")
WRITERS = {
    "trace_mega": [f"{r}-{c}" for r in ts.ROUTES for c in ("mega_lds", "mega_global", "spp2_centre_mega_lds")],
    "wf_nearest_flat": [f"A-{c}" for c in _WF_A],
    "wf_nearest_bvh": ["A-src9_bvh", "A-src7_bvh"],
    "wf_nearest_prefix": ["A-src8_prefix"],
    "wf_nearest_q4": ["A-src25_q4", "A-src26_q4"],
    "wf_fold": [f"{r}-{c}" for r in "BC" for c in _FOLD],
    "wf_tail": [f"{r}-{c}" for r in "BC" for c in ("tail1", "tail1_compose1")],
    "wf_output": [f"A-{c}" for c in ("compose1", "tail1_compose1", "src8_compose1", "spp2_centre_compose1")]
                 + [f"{r}-{c}" for r in ts.ROUTES for c in _RESOLVE],
    "path_kernel (HBM copy)": [f"{r}-{c}" for r in ts.ROUTES for c in ("path", "spp2_centre_path", "spp2_random_path")],
}
# The background scenes' pixels are the host's (bg_rgb, bg_bgr: no device table) on the wavefront, with and
# without compose; the path kernel computes its own and quantises them through its HBM copy.
BACKGROUND_WRITERS = {"host": [f"{spp}-{how}" for spp in (1, 2, 3) for how in ("wavefront", "wavefront_compose1")],
                      "path_kernel (HBM copy)": [f"{spp}-path" for spp in (1, 2, 3)]}


BACKGROUND_HOW, BACKGROUND_SPP = ("wavefront", "wavefront_compose1", "path"), (1, 2, 3)


def test_writer_table_names_real_cases():
    ids = {f"{r}-{c}" for r in ts.ROUTES for c in CASE_NAMES}
    assert len(WRITERS) == 9
    named = [x for v in WRITERS.values() for x in v]
    assert set(named) <= ids and len(named) == len(set(named))
    assert set(named) == ids, sorted(ids - set(named))       # every case's threshold pixels have one writer copy
    assert sorted(x for v in BACKGROUND_WRITERS.values() for x in v) == sorted(
        f"{spp}-{how}" for spp in BACKGROUND_SPP for how in BACKGROUND_HOW)


def _check(rgb, bgr, rays, shadow_rays, ref):
    bad8 = bgr != ref["bgr"]
    assert not bad8.any(), f"{bad8.sum()} BGR bytes of {bad8.size} differ from the oracle's"
    bad32 = ~om.same_f32(rgb, ref["rgb32"])
    assert not bad32.any(), f"{bad32.sum()} f32 values of {bad32.size} differ from the oracle's bits"
    assert (rays, shadow_rays) == (ref["counts"]["rays"], ref["counts"]["shadow_rays"])


@pytest.mark.parametrize("case", CASES, ids=CASE_NAMES)
@pytest.mark.parametrize("route", ts.ROUTES)
def test_threshold_scene(gpu_ctx, route, case):
    """Bytes, f32 bits and ray counts of the oracle: no tolerance, no pow result survives in these scenes."""
    ref = oracle(route, case["spp"], case["jitter"])
    spec = ts.scene(route, case["spp"])
    o = lr.render_opts(spec.width, spec.height, max_depth=spec.max_depth, spp=case["spp"], algo=case["algo"],
                       jitter=case["jitter"], seed=SEED)
    with tuning(gpu_ctx, **case["tune"]):
        gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))          # (the grids' knobs take effect here)
        if case["accum"]:
            with gpu_ctx.accumulator(o) as acc:
                rays = shadow = 0
                for _ in range(2):
                    acc.add(1, case["algo"])
                    st = gpu_ctx.stats()
                    rays, shadow = rays + st.rays, shadow + st.shadow_rays
                assert acc.samples == 2
                rgb, bgr = acc.resolve()
        else:
            rgb, bgr, st = gpu_ctx.render(o)
            rays, shadow = st.rays, st.shadow_rays
    _check(rgb, bgr, rays, shadow, ref)


@pytest.mark.parametrize("how", BACKGROUND_HOW)
@pytest.mark.parametrize("spp", BACKGROUND_SPP)
def test_background_pixels(gpu_ctx, spp, how):
    """The pixels the host computes (bg_rgb, bg_bgr): eight backgrounds that are threshold triples."""
    algo, tune = {"wavefront": (WF, {}), "wavefront_compose1": (WF, dict(compose=1)), "path": (PATH, {})}[how]
    for k, spec in enumerate(ts.background_scenes()):
        spec.antialias = spp
        key = ("bg", k, spp)
        if key not in _refs:
            _refs[key] = ref64.render(spec)
        ref = _refs[key]
        bg = (ref["rgb64"] == ref["rgb64"][0, 0]).all(axis=2)
        assert bg.sum() >= 100
        with tuning(gpu_ctx, **tune):
            gpu_ctx.upload(lr.Scene.deserialize(spec.to_text()))
            rgb, bgr, st = gpu_ctx.render(lr.render_opts(spec.width, spec.height, max_depth=spec.max_depth, spp=spp, algo=algo))
        got8 = bgr.reshape(spec.height, spec.width, 3)[bg]
        want8 = ref["bgr"].reshape(spec.height, spec.width, 3)[bg]
        assert np.array_equal(got8, want8), (k, got8[0], want8[0])
        assert om.same_f32(rgb[bg], ref["rgb32"][bg]).all(), k
        assert (st.rays, st.shadow_rays) == (ref["counts"]["rays"], ref["counts"]["shadow_rays"])
