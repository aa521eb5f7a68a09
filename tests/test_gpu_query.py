"""Ray queries on the device (rt_query_nearest / rt_query_occluded and their device variants, csrc/wf_query.hip)
against the Python model (tests/query_model.py, pinned against the oracle by test_query_model.py).

Required equal, with no tolerance: every f64 bit for bit (uint64 views; a NaN by its position: IEEE leaves a NaN's
sign and payload open, and the model's NaN comes from the host's 0/0), the object ids, the occlusion bytes, and
rays / shadow_rays / pixels / traced_rays / chunks and the work counters of rt_ctx_stats.  A last bit that differs is
a finding about the kernel, not a reason for a tolerance.

Ray sets, built on the host from the scenes of aov_model.SCENE_NAMES (at most 64 x 64):
  cam     (i)   the centre-jitter camera rays
  sur     (ii)  from every first hit the shadow ray to each point and directional light, with its squared range,
                and the mirror ray: origins on surfaces, the rays the renderer really issues
  scaled  (iii) (i) and (ii) with per-ray direction scales 2^k, k in {-40, -21, -20, -1, 0, 1, 20, 21, 40}: both sides
                of the slab tests' 2^+-20 switch
  edge          (i) and (ii) with every direction rescaled so that its largest component sits at the edge of the
                domain, 2^+-256 (alternating): the bound the culling argument gives
  far     (iv)  the camera rays started 2^21 (1 + extent) back along their own line: beyond the culling domain
                (the scene "far" is far_scenes.telephoto, whose camera is out there by itself)
  perm    (v)   a fixed permutation of (i)
No ray outside the domain the header states is sent to the device.
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
from oracle import ref64

import aov_model as am
import query_model as qm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAREST_LINE = re.compile(r"rtamd: query nearest src (\d+) rays (\d+) channels 0x([0-9a-f]+) workgroups (\d+)")
OCCLUDED_LINE = re.compile(r"rtamd: query occluded src (\d+) rays (\d+) range (\d) workgroups (\d+)")
NAMES = ("t", "object", "normal")
BIT = {"t": lr.RT_HIT_T, "object": lr.RT_HIT_OBJECT, "normal": lr.RT_HIT_NORMAL}


@pytest.fixture(scope="module")
def specs(tmp_path_factory):
    d = tmp_path_factory.mktemp("query_sky")
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


def upload(ctx, spec):
    ctx.upload(lr.Scene.deserialize(spec.to_text()))


def ranges_for(t, seed):
    """Squared ranges around the hits of a set that has none of its own: (t f)^2 with f in [0.5, 1.5), 1 for a miss."""
    f = np.random.default_rng(seed).uniform(0.5, 1.5, t.shape[0])
    with np.errstate(all="ignore"):
        r2 = (t * f) * (t * f)
    return np.where(np.isfinite(r2), r2, 1.0)


_SETS = {}


def ray_sets(spec):
    """{set: (rays [n, 6], r2 [n])} of a scene, built once (the model answers are built once too: expect())."""
    key = spec.to_text()
    if key in _SETS:
        return _SETS[key]
    cam = qm.camera_set(spec)
    tcam = qm.nearest(spec, cam)["t"]
    sur, sur_r2 = qm.surface_set(spec, cam)
    base = np.concatenate([cam, sur])
    base_r2 = np.concatenate([ranges_for(tcam, 1), sur_r2])
    scaled, scaled_r2, _ = qm.scaled_set(base, base_r2)
    edge, edge_r2, _ = qm.edge_set(base, base_r2)
    far = qm.far_set(spec, cam)
    assert (np.abs(far[:, :3]).max(axis=1) > lr.cull_reach(qm.extent(spec))).all() and qm.scene_in_domain(spec)
    perm = qm.permuted(cam.shape[0])
    sets = {"cam": (cam, base_r2[:cam.shape[0]]), "sur": (sur, sur_r2), "scaled": (scaled, scaled_r2),
            "edge": (edge, edge_r2),
            "far": (far, ranges_for(qm.nearest(spec, far)["t"], 2)), "perm": (cam[perm], base_r2[:cam.shape[0]][perm])}
    for name, (r, r2) in sets.items():
        assert qm.in_domain(r, r2).all(), name
    _SETS[key] = {k: (np.ascontiguousarray(r), np.ascontiguousarray(r2)) for k, (r, r2) in sets.items()}
    return _SETS[key]


_WANT = {}


def expect(spec, rays, r2, key=None):
    """The model's answers for one ray set: nearest, occlusion without a range, occlusion with r2 (one fold)."""
    if key is not None and key in _WANT:
        return _WANT[key]
    obj, t, nrm = qm.intersect(spec, rays)
    has = obj >= 0
    with np.errstate(all="ignore"):
        ranged = (has & (t * t < r2)).astype(np.uint8)
    want = ({"t": np.where(has, t, np.inf), "object": obj, "normal": np.where(has[:, None], nrm, 0.0)},
            has.astype(np.uint8), ranged)
    if key is not None:
        _WANT[key] = want
    return want


def same64(g, w):
    g, w = np.ascontiguousarray(g, np.float64), np.ascontiguousarray(w, np.float64)
    ng, nw = np.isnan(g), np.isnan(w)
    return g.shape == w.shape and np.array_equal(ng, nw) and np.array_equal(g.view(np.uint64)[~ng], w.view(np.uint64)[~nw])


def same(got, want, what=""):
    """Device arrays against the model's (or another query's): bits, NaN positions, ids."""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name in got:
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if name == "object":
            assert np.array_equal(g, w), (what, name, int((g != w).sum()))
        else:
            assert same64(g, w), (what, name, int((np.isnan(g) != np.isnan(w)).sum()),
                                  int((g.view(np.uint64) != w.view(np.uint64)).sum()))


def check_stats(st, n, shadow):
    assert (st.rays, st.traced_rays, st.shadow_rays, st.pixels, st.chunks) == (n, n, n if shadow else 0, 0, 0), \
        (st.rays, st.traced_rays, st.shadow_rays, st.pixels, st.chunks)
    assert (st.box_tests, st.sphere_tests, st.shadow_box_tests, st.shadow_sphere_tests) == (0, 0, 0, 0)


def nearest(ctx, capfd, rays, channels=lr.RT_HIT_ALL, out=None, flags=0):
    """One rt_query_nearest under tuning verbose -> (arrays, the source and the workgroups its verbose line names)."""
    n = qm.as_rays(rays).shape[0]
    with tuning(ctx, verbose=1):
        capfd.readouterr()
        arrays, st = ctx.query_nearest(rays, channels, out=out, flags=flags)
        err = capfd.readouterr().err
    lines = NEAREST_LINE.findall(err)
    assert len(lines) == 1 and not OCCLUDED_LINE.findall(err), err
    src, ln, lch, G = int(lines[0][0]), int(lines[0][1]), int(lines[0][2], 16), int(lines[0][3])
    assert (ln, lch) == (n, channels), err
    check_stats(st, n, False)
    return arrays, src, G


def occluded(ctx, capfd, rays, r2=None, out=None, flags=0):
    n = qm.as_rays(rays).shape[0]
    with tuning(ctx, verbose=1):
        capfd.readouterr()
        occ, st = ctx.query_occluded(rays, r2, out=out, flags=flags)
        err = capfd.readouterr().err
    lines = OCCLUDED_LINE.findall(err)
    assert len(lines) == 1 and not NEAREST_LINE.findall(err), err
    src, ln, lr_, G = (int(x) for x in lines[0])
    assert (ln, lr_) == (n, 0 if r2 is None else 1), err
    check_stats(st, n, True)
    return occ, src, G


def check_all(ctx, capfd, spec, rays, r2, what, key=None):
    """The three queries of one ray set against the model -> (nearest source, occlusion source)."""
    want, want_any, want_ranged = expect(spec, rays, r2, key)
    got, src, _ = nearest(ctx, capfd, rays)
    same(got, want, what)
    occ, src_occ, _ = occluded(ctx, capfd, rays)
    assert occ.dtype == np.uint8 and np.array_equal(occ, want_any), (what, "no range", int((occ != want_any).sum()))
    occ, src_occ2, _ = occluded(ctx, capfd, rays, r2)
    assert np.array_equal(occ, want_ranged), (what, "range", int((occ != want_ranged).sum()))
    assert src_occ == src_occ2
    return src, src_occ


# ---- 1. every scene, every ray set ---------------------------------------------------------------

@pytest.mark.parametrize("name", am.SCENE_NAMES)
def test_scene_matches_the_model(gpu_ctx, capfd, specs, name):
    spec = specs[name]
    upload(gpu_ctx, spec)
    for sname, (rays, r2) in ray_sets(spec).items():
        check_all(gpu_ctx, capfd, spec, rays, r2, (name, sname), key=(name, sname))


def test_the_sets_exercise_both_answers(specs):
    """(host only) the sets are not trivially all-hit or all-miss, and ranges decide some rays."""
    hit = miss = decided = nan = 0
    for name in ("random", "extreme", "nan_plane", "far"):
        for sname, (rays, r2) in ray_sets(specs[name]).items():
            want, any_, ranged = expect(specs[name], rays, r2, (name, sname))
            hit += int(any_.sum()); miss += int((1 - any_).sum()); decided += int((any_ != ranged).sum())
            nan += int(np.isnan(want["t"]).sum())
    assert hit > 1000 and miss > 1000 and decided > 500 and nan > 0


# ---- 2. tied to the first-hit feature buffers -------------------------------------------------------

@pytest.mark.parametrize("name", am.SCENE_NAMES)
def test_camera_rays_equal_the_aov_render(gpu_ctx, capfd, specs, name):
    spec = specs[name]
    upload(gpu_ctx, spec)
    rays = ray_sets(spec)["cam"][0]
    got, _, _ = nearest(gpu_ctx, capfd, rays)
    aov, _ = gpu_ctx.render_aov(lr.render_opts(spec.width, spec.height, spp=1, jitter=am.CENTER),
                                lr.RT_AOV_DEPTH | lr.RT_AOV_NORMAL | lr.RT_AOV_OBJECT)
    hit = got["object"] >= 0
    assert np.array_equal(got["object"], aov["object"].reshape(-1))
    assert np.isposinf(got["t"][~hit]).all() and not aov["depth"].reshape(-1)[~hit].any()
    depth = np.where(hit, got["t"], 0.0).astype(np.float32)                  # the AOV's 0.0 for a miss, +inf here
    nd, na = np.isnan(depth), np.isnan(aov["depth"].reshape(-1))
    assert np.array_equal(nd, na) and np.array_equal(am.bits(depth)[~nd], am.bits(aov["depth"].reshape(-1))[~na])
    nrm = qm.flip(got["normal"], rays).astype(np.float32)                    # raytrace.rs:38, then one rounding
    assert np.array_equal(am.bits(nrm), am.bits(aov["normal"].reshape(-1, 3))), name


# ---- 3. the range's edge -------------------------------------------------------------------------

def test_the_ranges_edge(gpu_ctx, capfd, specs):
    spec = specs["random"]
    upload(gpu_ctx, spec)
    rays, _ = ray_sets(spec)["cam"]
    got, _, _ = nearest(gpu_ctx, capfd, rays)
    hit = got["object"] >= 0
    assert hit.sum() > 500 and (~hit).sum() > 100
    hr, t = np.ascontiguousarray(rays[hit]), got["t"][hit]
    tt = t * t
    assert not occluded(gpu_ctx, capfd, hr, tt)[0].any()                     # t*t < t*t is false
    assert occluded(gpu_ctx, capfd, hr, np.nextafter(tt, np.inf))[0].all()
    assert not occluded(gpu_ctx, capfd, hr, np.zeros(hr.shape[0]))[0].any()
    assert occluded(gpu_ctx, capfd, hr, np.full(hr.shape[0], np.inf))[0].all()
    assert not occluded(gpu_ctx, capfd, rays[~hit], np.full(int((~hit).sum()), np.inf))[0].any()
    # a plane's NaN t: occluded without a range, not under any range
    spec = specs["nan_plane"]
    upload(gpu_ctx, spec)
    rays, _ = ray_sets(spec)["cam"]
    got, _, _ = nearest(gpu_ctx, capfd, rays)
    nan = np.isnan(got["t"])
    assert nan.sum() > 10 and (got["object"][nan] >= 0).all()
    assert np.array_equal(got["normal"][nan], np.broadcast_to([0.0, 1.0, 0.0], (int(nan.sum()), 3)))
    assert occluded(gpu_ctx, capfd, rays)[0][nan].all()
    for r2 in (np.full(rays.shape[0], np.inf), np.full(rays.shape[0], 1e300), np.zeros(rays.shape[0])):
        assert not occluded(gpu_ctx, capfd, rays, r2)[0][nan].any()


# ---- 4. every source family ----------------------------------------------------------------------

SMALL = lambda: scenes.random_spheres(200, 64, 48, 4, seed=11, name="sources")                       # noqa: E731
BIG = lambda: scenes.random_spheres(2500, 64, 48, 4, seed=12, box_scale=2.0, name="sources_big")     # noqa: E731
# (scene, tuning) -> the (nearest, occlusion) sources that must run; test_gpu_sources.py's scenes: 200 spheres fit
# LDS whole, 2500 do not (nor does their tree), and the prefix sources get a 1 KB prefix so that most of the tree is
# below it.  The camera's view grid (cam 3 / -1: 22 / 23 for the AOV) and the light grids are never a query's.
AUTO = None
FAMILIES = [
    ("small", dict(), (9, 10)), ("small", dict(cam=3), (9, 10)), ("small", dict(cam=-1), (9, 10)),
    ("small", dict(src=7, src_occ=7), (7, 7)), ("small", dict(src=2, src_occ=2), (2, 2)),
    ("small", dict(src=8, src_occ=8, prefix_kb=1), (8, 8)), ("small", dict(src=1, src_occ=1), (1, 1)),
    ("small", dict(src=0, src_occ=0), (0, 0)), ("small", dict(src=9, src_occ=14), (9, 10)),
    # AUTO: the scene's automatic choice (a binary16 prefix source, 5 or 6 by the tree's depth), which the quantised
    # tree's numbers (25, 26: no instantiation here) fall back to
    ("big", dict(), (AUTO, 11)), ("big", dict(cam=3), (AUTO, 11)), ("big", dict(cam=-1), (AUTO, 11)),
    ("big", dict(src=6, src_occ=8, prefix_kb=1), (6, 8)), ("big", dict(src=5, src_occ=15, prefix_kb=1), (5, 11)),
    ("big", dict(src=8, src_occ=2, prefix_kb=1), (8, 2)), ("big", dict(src=2, src_occ=1), (2, 0)),
    ("big", dict(src=1, src_occ=0), (0, 0)), ("big", dict(src=25), (AUTO, 11)), ("big", dict(src=26, src_occ=26), (AUTO, 11)),
]


@pytest.mark.parametrize("scene", ["small", "big"])
def test_every_source_family_agrees(gpu_ctx, capfd, scene):
    spec = SMALL() if scene == "small" else BIG()
    upload(gpu_ctx, spec)
    sets = ray_sets(spec)
    step = 1 if scene == "small" else 3                       # (2500 objects in the model: a third of the rays)
    pick = [("cam", step), ("scaled", 2 * step), ("edge", 2 * step)]
    rays = np.ascontiguousarray(np.concatenate([sets[k][0][::st] for k, st in pick]))
    r2 = np.ascontiguousarray(np.concatenate([sets[k][1][::st] for k, st in pick]))
    ran, ran_occ, auto = set(), set(), None
    for sc, tune, (src_want, occ_want) in FAMILIES:
        if sc != scene:
            continue
        with tuning(gpu_ctx, **tune):
            src, src_occ = check_all(gpu_ctx, capfd, spec, rays, r2, (scene, tune), key=("families", scene))
        if src_want is AUTO:
            auto = src if auto is None else auto
            assert auto in (5, 6)
            src_want = auto
        assert (src, src_occ) == (src_want, occ_want), (tune, src, src_occ)
        assert src not in (22, 23) and src_occ not in (14, 15)
        ran.add(src)
        ran_occ.add(src_occ)
    assert ran == ({9, 7, 2, 8, 1, 0} if scene == "small" else {5, 6, 8, 2, 0}), ran
    assert ran_occ == ({10, 7, 2, 8, 1, 0} if scene == "small" else {11, 8, 2, 0}), ran_occ


# ---- 5. sizes --------------------------------------------------------------------------------------

SENT_F, SENT_I, SENT_B, PAD = -12345.5, -777, 0xAB, 64


def padded(n):
    return {"t": np.full(n + PAD, SENT_F, np.float64), "object": np.full(n + PAD, SENT_I, np.int32),
            "normal": np.full(3 * (n + PAD), SENT_F, np.float64)}


def check_sized(ctx, capfd, rays, r2, want, want_any, want_ranged, channels=lr.RT_HIT_ALL):
    """Queries into buffers 64 elements longer than needed: the answers, the untouched tail, the untouched
    unselected buffers -> the workgroups of the nearest launch."""
    n = rays.shape[0]
    out = padded(n)
    got, _, G = nearest(ctx, capfd, rays, channels, out=out)
    for name in NAMES:
        k = 3 if name == "normal" else 1
        sent = SENT_I if name == "object" else SENT_F
        if channels & BIT[name]:
            body = out[name][:n * k].reshape((n, 3) if k == 3 else (n,))
            same({name: body}, {name: want[name]}, (n, name))
            assert (out[name][n * k:] == sent).all(), (n, name, "wrote past its end")
        else:
            assert (out[name] == sent).all(), (n, name, "written though not selected")
    for rr, w in ((None, want_any), (r2, want_ranged)):
        occ = np.full(n + PAD, SENT_B, np.uint8)
        occluded(ctx, capfd, rays, rr, out=occ)
        assert np.array_equal(occ[:n], w) and (occ[n:] == SENT_B).all(), (n, rr is None)
    return G


def test_sizes_tails_and_masks(gpu_ctx, capfd):
    spec = SMALL()
    upload(gpu_ctx, spec)
    sets = ray_sets(spec)
    base = np.ascontiguousarray(np.concatenate([sets["far"][0], sets["scaled"][0]])[:4096])
    base_r2 = np.ascontiguousarray(np.concatenate([sets["far"][1], sets["scaled"][1]])[:4096])
    assert base.shape[0] == 4096
    want, want_any, want_ranged = expect(spec, base, base_r2)
    for n in (0, 1, 63, 64, 65, 1023, 1024, 1025):
        G = check_sized(gpu_ctx, capfd, base[:n], base_r2[:n], {k: v[:n] for k, v in want.items()}, want_any[:n],
                        want_ranged[:n])
        assert G == (n + 1023) // 1024, (n, G)
    for mask in (lr.RT_HIT_T, lr.RT_HIT_OBJECT, lr.RT_HIT_NORMAL, lr.RT_HIT_T | lr.RT_HIT_NORMAL,
                 lr.RT_HIT_OBJECT | lr.RT_HIT_NORMAL):
        check_sized(gpu_ctx, capfd, base[:1025], base_r2[:1025], {k: v[:1025] for k, v in want.items()},
                    want_any[:1025], want_ranged[:1025], channels=mask)
    # buffers of channels that are not selected may be absent altogether
    got, _, _ = nearest(gpu_ctx, capfd, base[:65], lr.RT_HIT_OBJECT)
    assert set(got) == {"object"} and np.array_equal(got["object"], want["object"][:65])
    # more rays than the grid has work-items: the grid-stride loop's second trip.  The grid's size comes from a
    # query that is certainly larger (on the empty scene: nothing to walk), then n = G * 1024 + 1025 rays, the 4096
    # above repeated (the model's answers repeat with them)
    upload(gpu_ctx, am.adversarial_scenes.tiny())
    _, _, G = nearest(gpu_ctx, capfd, np.resize(base, (1 << 20, 6)), lr.RT_HIT_OBJECT)
    assert 64 <= G < 1024, G
    upload(gpu_ctx, spec)
    n = G * 1024 + 1025
    idx = np.arange(n) % 4096
    G2 = check_sized(gpu_ctx, capfd, np.ascontiguousarray(base[idx]), base_r2[idx], {k: v[idx] for k, v in want.items()},
                     want_any[idx], want_ranged[idx])
    assert G2 == G and G * 1024 < n


# ---- 6. the device variants on a torch stream ------------------------------------------------------

_DEVICE = r"""
import sys
sys.path[:0] = sys.argv[1:4]
import numpy as np
import torch                      # first: the process then uses torch's HIP runtime for both
import libraytrace as lr
from libraytrace import scenes
import query_model as qm

spec = scenes.random_spheres(64, 64, 48, 4, seed=9, plane=True, name="aov_rand")
W, H = spec.width, spec.height
cam = qm.camera_set(spec)
sur, sur_r2 = qm.surface_set(spec, cam)
rays = np.ascontiguousarray(np.concatenate([cam, sur])[:5001])
n = rays.shape[0]
r2 = np.ascontiguousarray(np.concatenate([np.full(cam.shape[0], 30.0), sur_r2])[:n])
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(dev)               # not torch's default stream
assert stream.cuda_stream != 0
SENT = -777.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


with lr.Context(0) as ctx:
    ctx.upload(lr.Scene.deserialize(spec.to_text()))
    host, _ = ctx.query_nearest(rays)
    host_any, _ = ctx.query_occluded(rays)
    host_ranged, _ = ctx.query_occluded(rays, r2)
    assert (host["object"] >= 0).sum() > 1000 and host_any.sum() > 1000 and (host_any != host_ranged).sum() > 100
    colour = torch.zeros((H, 3 * W), dtype=torch.uint8, device=dev)
    with torch.cuda.stream(stream):
        d_all = torch.from_numpy(np.concatenate([np.zeros((1, 6)), rays])).to(dev)        # [n + 1, 6], ray 0 a dummy
        d_r2 = torch.from_numpy(r2).to(dev)
    stream.synchronize()
    assert d_all.data_ptr() % 16 == 0
    for mask in (lr.RT_HIT_ALL, lr.RT_HIT_T | lr.RT_HIT_OBJECT, lr.RT_HIT_NORMAL):
        t = {"t": torch.full((n,), SENT, dtype=torch.float64, device=dev),
             "object": torch.full((n,), -777, dtype=torch.int32, device=dev),
             "normal": torch.full((n, 3), SENT, dtype=torch.float64, device=dev)}
        occ = torch.full((2, n), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        # a colour render just before, on the context's own stream: the queries are ordered after it
        ctx.render_device(lr.render_opts(W, H, max_depth=4, spp=1, flags=lr.RT_OUT_BGR_U8), 0, colour.data_ptr())
        # the rays as a view offset by one ray (48 B): still 16-byte aligned
        d_rays = d_all[1:]
        assert d_rays.data_ptr() == d_all.data_ptr() + 48
        ctx.query_nearest_device(d_rays.data_ptr(), n, mask, {k: v.data_ptr() for k, v in t.items()}, stream.cuda_stream)
        st = ctx.stats()                      # synchronises with the query
        assert (st.rays, st.traced_rays, st.shadow_rays, st.pixels, st.chunks) == (n, n, 0, 0, 0), (st.rays, st.shadow_rays)
        ctx.query_occluded_device(d_rays.data_ptr(), 0, n, occ[0].data_ptr(), stream.cuda_stream)
        ctx.query_occluded_device(d_rays.data_ptr(), d_r2.data_ptr(), n, occ[1].data_ptr(), stream.cuda_stream)
        st = ctx.stats()
        assert (st.rays, st.traced_rays, st.shadow_rays, st.pixels, st.chunks) == (n, n, n, 0, 0), (st.rays, st.shadow_rays)
        stream.synchronize()
        for name, bit in (("t", 1), ("object", 2), ("normal", 4)):
            got = t[name].cpu().numpy()
            if not mask & bit:
                assert (got == (SENT if name != "object" else -777)).all(), (name, "written though not selected")
            elif name == "object":
                assert np.array_equal(got, host[name]), name
            else:
                nan = np.isnan(got)
                assert np.array_equal(nan, np.isnan(host[name])) and np.array_equal(bits(got)[~nan], bits(host[name])[~nan]), name
        got = occ.cpu().numpy()
        assert np.array_equal(got[0], host_any) and np.array_equal(got[1], host_ranged)
    # a view offset by one double (8 B) is refused, and is no render
    before = ctx.stats()
    flat = d_all.reshape(-1)
    for call in (lambda: ctx.query_nearest_device(flat[1:].data_ptr(), n, lr.RT_HIT_T, {"t": t["t"].data_ptr()}, stream.cuda_stream),
                 lambda: ctx.query_occluded_device(flat[1:].data_ptr(), 0, n, occ[0].data_ptr(), stream.cuda_stream)):
        try:
            call()
        except lr.RtError as e:
            assert e.code == lr.RT_E_INVALID and "aligned" in str(e), str(e)
        else:
            raise AssertionError("a misaligned d_rays was accepted")
    after = ctx.stats()
    assert (after.rays, after.shadow_rays) == (before.rays, before.shadow_rays)
    # the context's own stream (NULL) works as well
    ctx.query_occluded_device(d_all[1:].data_ptr(), 0, n, occ[0].data_ptr())
    ctx.stats()
    assert np.array_equal(occ[0].cpu().numpy(), host_any)
print("query_device ok")
"""


def test_device_buffers_on_a_torch_stream():
    """rt_query_nearest_device / rt_query_occluded_device on torch tensors and a non-default stream equal the host
    variants, bit for bit; unselected buffers keep their sentinel; the alignment rule.  In a child process: torch must
    initialise HIP before the library does."""
    out = subprocess.run([sys.executable, "-c", _DEVICE, ROOT, os.path.join(ROOT, "rust-raytrace_amd"),
                          os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "query_device ok" in out.stdout, out.stdout[-1000:] + out.stderr[-3000:]


# ---- 7. lifecycle and refusals ---------------------------------------------------------------------

def stats_tuple(st):
    return (st.rays, st.shadow_rays, st.pixels, st.traced_rays, st.chunks)


def test_refusals_leave_the_statistics_alone(gpu_ctx, capfd, specs):
    spec = specs["random"]
    upload(gpu_ctx, spec)
    rays, r2 = ray_sets(spec)["cam"]
    n = rays.shape[0]
    o = lr.render_opts(spec.width, spec.height, max_depth=spec.max_depth, spp=1)
    gpu_ctx.render(o)
    prev = stats_tuple(gpu_ctx.stats())
    assert prev[2] == spec.width * spec.height

    def refused(code, call):
        with pytest.raises(lr.RtError) as e:
            call()
        assert e.value.code == code, (e.value.code, code, str(e.value))
        assert stats_tuple(gpu_ctx.stats()) == prev

    inv = lr.RT_E_INVALID
    refused(inv, lambda: gpu_ctx.query_nearest(rays, 0))                                   # no channel
    refused(inv, lambda: gpu_ctx.query_nearest(rays, 8))                                   # unknown bits
    refused(inv, lambda: gpu_ctx.query_nearest(rays, lr.RT_HIT_ALL | 64))
    refused(inv, lambda: gpu_ctx.query_nearest(rays, lr.RT_HIT_T, out={}))                 # a selected channel's pointer is NULL
    refused(inv, lambda: gpu_ctx.query_nearest(rays, lr.RT_HIT_ALL, out={"t": np.zeros(n), "normal": np.zeros(3 * n)}))
    for fl in (lr.RT_COUNT_WORK, lr.RT_OUT_RGB_F32, lr.RT_TIME_KERNELS | lr.RT_OUT_BGR_U8, 1 << 20):
        refused(inv, lambda: gpu_ctx.query_nearest(rays, flags=fl))                        # unknown flag bits
        refused(inv, lambda: gpu_ctx.query_occluded(rays, flags=fl))
    P = lr.C.c_void_p
    bufs = lr.rt_hit_buffers()
    t = np.zeros(n)
    bufs.t = t.ctypes.data
    lib, h = lr.lib, gpu_ctx._h

    def raw(rc):
        if rc != lr.RT_OK:
            raise lr.RtError(rc, "")

    refused(inv, lambda: raw(lib.rt_query_nearest(h, None, n, lr.RT_HIT_T, lr.C.byref(bufs), 0, None)))       # NULL rays
    refused(inv, lambda: raw(lib.rt_query_nearest(h, P(rays.ctypes.data), n, lr.RT_HIT_T, None, 0, None)))    # NULL struct
    occ = np.zeros(n, np.uint8)
    refused(inv, lambda: raw(lib.rt_query_occluded(h, None, None, n, P(occ.ctypes.data), 0, None)))           # NULL rays
    refused(inv, lambda: raw(lib.rt_query_occluded(h, P(rays.ctypes.data), None, n, None, 0, None)))          # NULL occluded
    # the device entry points refuse the same way (nothing is launched: the pointers are never followed)
    refused(inv, lambda: gpu_ctx.query_nearest_device(0, n, lr.RT_HIT_T, {"t": 16}))
    refused(inv, lambda: gpu_ctx.query_nearest_device(4096, n, 0, {}))
    refused(inv, lambda: gpu_ctx.query_nearest_device(4096, n, lr.RT_HIT_T, {}))
    refused(inv, lambda: gpu_ctx.query_nearest_device(4096 + 8, n, lr.RT_HIT_T, {"t": 16}))                   # 8-byte aligned only
    refused(inv, lambda: gpu_ctx.query_occluded_device(4096 + 8, 0, n, 16))
    refused(inv, lambda: gpu_ctx.query_occluded_device(4096, 0, n, 0))
    refused(inv, lambda: gpu_ctx.query_occluded_device(4096, 0, n, 16, flags=lr.RT_COUNT_WORK))
    # no scene uploaded: RT_E_NOSCENE (after the argument checks)
    with lr.Context(0) as fresh:
        with pytest.raises(lr.RtError) as e:
            fresh.query_nearest(rays)
        assert e.value.code == lr.RT_E_NOSCENE
        with pytest.raises(lr.RtError) as e:
            fresh.query_occluded(rays)
        assert e.value.code == lr.RT_E_NOSCENE
        with pytest.raises(lr.RtError) as e:
            fresh.query_nearest(rays, 0)
        assert e.value.code == lr.RT_E_INVALID
    # n = 0 is a render: it launches nothing, looks at no pointer, and replaces the statistics
    assert lib.rt_query_nearest(h, None, 0, lr.RT_HIT_ALL, None, 0, None) == lr.RT_OK
    check_stats(gpu_ctx.stats(), 0, False)
    assert lib.rt_query_occluded_device(h, None, None, 0, None, 0, None) == lr.RT_OK
    check_stats(gpu_ctx.stats(), 0, True)


def test_queries_disturb_no_working_set(gpu_ctx, capfd, specs):
    spec = specs["random"]
    upload(gpu_ctx, spec)
    rays, r2 = ray_sets(spec)["sur"]
    o = lr.render_opts(spec.width, spec.height, max_depth=spec.max_depth, spp=1, algo=lr.RT_ALGO_WAVEFRONT)
    ref = ref64.render(spec)
    rgb0, bgr0, st0 = gpu_ctx.render(o)
    assert np.array_equal(bgr0, ref["bgr"]) and st0.rays == ref["counts"]["rays"] and st0.chunks >= 1
    gen0 = gpu_ctx.generation_counts()
    check_all(gpu_ctx, capfd, spec, rays, r2, "between renders", key=("random", "sur"))
    gpu_ctx.reserve(o, host=True)
    check_all(gpu_ctx, capfd, spec, rays, r2, "between reserve and render", key=("random", "sur"))
    rgb1, bgr1, st1 = gpu_ctx.render(o)
    assert np.array_equal(bgr1, ref["bgr"]) and np.array_equal(bgr0, bgr1) and np.array_equal(am.bits(rgb0), am.bits(rgb1))
    assert stats_tuple(st0) == stats_tuple(st1) and gpu_ctx.generation_counts() == gen0
    # an accumulator alive across a query keeps its sums
    oa = lr.render_opts(spec.width, spec.height, max_depth=2, jitter=am.RANDOM, seed=5)
    with gpu_ctx.accumulator(oa) as acc:
        acc.add(2, algo=lr.RT_ALGO_PATH)
        before, _ = acc.download()
        check_all(gpu_ctx, capfd, spec, rays, r2, "beside an accumulator", key=("random", "sur"))
        after, ns = acc.download()
        assert ns == 2 and np.array_equal(before.view(np.uint64), after.view(np.uint64))


def test_kernel_times_and_statistics_read_late(gpu_ctx, specs):
    spec = specs["random"]
    upload(gpu_ctx, spec)
    rays, r2 = ray_sets(spec)["cam"]
    n = rays.shape[0]
    gpu_ctx.kernel_times()
    gpu_ctx.query_nearest(rays, flags=lr.RT_TIME_KERNELS, stats=False)
    gpu_ctx.query_occluded(rays, r2, flags=lr.RT_TIME_KERNELS, stats=False)
    gpu_ctx.query_nearest(rays, lr.RT_HIT_T, stats=False)                   # not timed
    gpu_ctx.query_occluded(rays, stats=False)                               # not timed
    for _ in range(2):                                                      # as often as wanted
        check_stats(gpu_ctx.stats(), n, True)
    kt = gpu_ctx.kernel_times()
    assert kt["nearest"][1] == 1 and kt["nearest"][0] > 0, kt
    assert kt["occlusion"][1] == 1 and kt["occlusion"][0] > 0, kt
    assert sum(v[1] for v in kt.values()) == 2, kt
    upload(gpu_ctx, specs["tiny"])                  # another scene: the statistics stay the last render's
    check_stats(gpu_ctx.stats(), n, True)


def test_another_scene_answers_for_itself(gpu_ctx, capfd, specs):
    a, b = specs["random"], specs["inside"]
    rays, r2 = ray_sets(a)["cam"]
    upload(gpu_ctx, a)
    check_all(gpu_ctx, capfd, a, rays, r2, "first scene", key=("random", "cam"))
    upload(gpu_ctx, b)
    want_b = expect(b, rays, r2)
    check_all(gpu_ctx, capfd, b, rays, r2, "second scene, the first one's rays")
    assert not np.array_equal(want_b[0]["object"], expect(a, rays, r2, ("random", "cam"))[0]["object"])
    upload(gpu_ctx, am.adversarial_scenes.tiny())   # nothing to hit
    got, _, _ = nearest(gpu_ctx, capfd, rays)
    assert (got["object"] == -1).all() and np.isposinf(got["t"]).all() and not got["normal"].any()
    assert not occluded(gpu_ctx, capfd, rays)[0].any()
