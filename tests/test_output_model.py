"""output_model.py, the numpy restatement of the output stage that test_gpu_output.py holds the device to,
pinned on the CPU three ways -- quantise to the oracle's and the host's to_srgb on the probe's operands, to_f32
to an integer-arithmetic rounding, the whole rule to ref_render's own rgb32 and bgr -- together with the
coverage conditions of the probe's operands and of the threshold scenes (threshold_scenes.py), asserted on
the model and on the oracle's output: a scene or an operand set that stops delivering exact thresholds fails
here, without a GPU."""
import numpy as np
import pytest

from oracle import ref64

import output_model as om
import threshold_scenes as ts

try:
    import libraytrace as lr
except ImportError:                # the host library is not built: the oracle alone is the authority
    lr = None


@pytest.fixture(scope="module")
def probes():
    return {n: om.probe_sums(n) for n in om.SAMPLES}


def test_table_is_the_pinned_one():
    """The thresholds are the oracle's averages table (tests/golden/srgb_tables.json pins it in test_oracle.py),
    and the 510 values are distinct, positive and below 1."""
    t = om.threshold_values()
    assert t.shape == (255, 2) and len(np.unique(t)) == 510
    assert (t > 0).all() and (t < 1).all() and (t[:, 1] < t[:, 0]).all()
    assert (om.ordinal(t[:, 0]) - om.ordinal(t[:, 1]) == 1).all()
    assert om.quantise(t[:, 0]).tolist() == list(range(1, 256)) and om.quantise(t[:, 1]).tolist() == list(range(255))


def test_quantise_is_to_srgb_on_the_probes_operands(probes):
    """Every distinct quotient of the probe, through the oracle's to_srgb and, where the library loads, the
    host's."""
    q = np.unique(np.concatenate([om.average(s, n) for n, (s, _, _) in probes.items()]).view(np.uint64)).view(np.float64)
    assert q.size > 20000
    got = om.quantise(q)
    assert got.tolist() == [ref64.to_srgb(x) for x in q]
    if lr is not None:
        assert got.tolist() == [lr.to_srgb(x) for x in q]
    assert om.quantise(np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0])).tolist() == [255, 255, 255, 0, 0, 0]


def test_which_edits_of_the_device_search_change_it(probes):
    """The device's to_srgb is a guard and eight halvings.  Restated on the probe's quotients: it is the
    quantiser; so are the eight halvings WITHOUT the guard (a value at or above T_254, and NaN, is never
    `<`, and walks lo up to 255), so the guard is an early exit and rewriting it as `v >= T_254` changes no
    result -- that edit cannot fail any test.  Seven halvings are not the quantiser."""
    q = np.unique(np.concatenate([om.average(s, n) for n, (s, _, _) in probes.items()]).view(np.uint64)).view(np.float64)
    want = om.quantise(q)
    assert np.isnan(q).sum() >= 3 and np.array_equal(om.binary_search(q), want)
    assert np.array_equal(om.binary_search(q, guard=False), want)
    assert np.array_equal(om.binary_search(q, guard_ge=True), want)
    assert (om.binary_search(q, turns=7) != want).sum() > 1000


def test_to_f32_is_the_integer_rounding(probes):
    """numpy's cast against mantissa bits, guard, sticky and ties to even, on every quotient of the tie,
    denormal, flush and overflow classes (and a sample of the rest)."""
    q = np.concatenate([om.average(s, n) for n, (s, _, _) in probes.items()])
    q = np.unique(q.view(np.uint64)).view(np.float64)
    cls = om.f32_class(q)
    pick = np.zeros(q.shape, bool)
    for name in om.CLASSES:
        assert cls[name].sum() >= 100, name
        pick |= cls[name]
    pick[::7] = True
    x = q[pick]
    assert x.size > 8000
    want = om.to_f32_bits_integer(x)
    got = om.f32_bits(om.to_f32(x))
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan]) and np.isnan(om.to_f32(x[nan])).all()
    # the named corners
    for v, bits in ((om.F32_OVERFLOW_TIE, 0x7F800000), (om.step(om.F32_OVERFLOW_TIE, -1), 0x7F7FFFFF),
                    (-om.F32_OVERFLOW_TIE, 0xFF800000), (2.0 ** -150, 0), (om.step(2.0 ** -150, 1), 1),
                    (-(2.0 ** -150), 0x80000000), (3.0 * 2.0 ** -150, 2), (2.0 ** -126 - 2.0 ** -150, 0x00800000),
                    (1.0 + 2.0 ** -24, 0x3F800000), (1.0 + 3.0 * 2.0 ** -24, 0x3F800002), (-0.0, 0x80000000)):
        assert int(om.to_f32_bits_integer(np.array([v]))[0]) == bits == int(om.f32_bits(om.to_f32(np.array([v])))[0]), v


def test_probe_operands_sit_where_they_should(probes):
    """For every divisor: both bytes i and i + 1 occur among the quotients within two values of T_i, for
    every i; every f32 class holds at least 100 records; the specials are there."""
    for n, (sums, tgt, lab) in probes.items():
        cov = om.threshold_coverage(sums, n)
        assert cov.all(), (n, np.argwhere(~cov)[:5])
        q = om.average(sums, n)
        cls = om.f32_class(q)
        for name in om.CLASSES:
            assert cls[name].sum() >= 100, (n, name, int(cls[name].sum()))
        assert np.isnan(q).sum() >= 1 and np.isposinf(q).sum() >= 1 and np.isneginf(q).sum() >= 1
        assert (q == 1.0).any() and (om.f32_bits(om.to_f32(q)) == 0x80000000).any() and (q < 0).sum() > 100
        assert ((q != 0) & (np.abs(q) < 2.0 ** -1022)).sum() >= 100, n          # f64 denormal quotients
        assert set(om.quantise(q).tolist()) == set(range(256))
        if n & (n - 1) == 0:       # the quotient of an exact product is the target itself
            aimed = ~np.isnan(tgt)
            assert np.array_equal(q[aimed].view(np.uint64), tgt[aimed].view(np.uint64))
    assert (om.average(probes[2 ** 31][0], 2 ** 31) == 2.0 ** -1074).any()


def test_quantising_the_f32_would_differ():
    """The rule's point: about half of the values just below a threshold round UP to f32 across it, so
    quantising the f32-rounded colour gives another byte there (what the probe and the scenes must see)."""
    below = om.threshold_values()[:, 1]
    wrong = om.quantise(om.to_f32(below).astype(np.float64)) != om.quantise(below)
    assert 64 <= wrong.sum() <= 192, wrong.sum()


@pytest.fixture(scope="module")
def renders():
    out = {}
    for route in ts.ROUTES:
        out[route, 1, 0] = ref64.render(ts.scene(route, 1))
        out[route, 2, 0] = ref64.render(ts.scene(route, 2))
        out[route, 2, 1] = ref64.render(ts.scene(route, 2), jitter=1, seed=7, rng=1)
    return out


@pytest.mark.parametrize("route", ts.ROUTES)
def test_threshold_scenes_deliver_every_value(renders, route):
    """All 510 values appear exactly in the oracle's rgb64 on every route, at spp 1, at spp 2 with centre
    jitter ((0 + v + v) / 2 is exact) and with random jitter; on at least 64 pixels per sphere; route C on
    mirror pixels alone (the plane fills the view: every camera ray starts a chain)."""
    for key in ((route, 1, 0), (route, 2, 0), (route, 2, 1)):
        r = renders[key]
        assert ts.values_present(r["rgb64"]).all(), key
        assert ts.pixels_per_triple(r["rgb64"]).min() >= 64, key
    spp1 = renders[route, 1, 0]
    assert np.array_equal(spp1["rgb64"], renders[route, 2, 0]["rgb64"])
    px = ts.WIDTH * ts.HEIGHT
    want = {"A": (px, 0), "B": None, "C": (3 * px, px)}[route]        # C: camera, mirror and light rays for all
    if want:
        assert (spp1["counts"]["rays"], spp1["counts"]["shadow_rays"]) == want
    else:
        lit = int((spp1["rgb64"] != np.array(ts.BACKGROUND)).any(axis=2).sum())
        assert (spp1["counts"]["rays"], spp1["counts"]["shadow_rays"]) == (px + lit, lit)
    # the three routes show the same frame
    assert np.array_equal(spp1["rgb64"], renders["A", 1, 0]["rgb64"])


def test_model_is_the_oracles_output_on_the_threshold_scenes(renders):
    for key, r in renders.items():
        assert om.same_f32(om.to_f32(r["rgb64"]), r["rgb32"]).all(), key
        assert np.array_equal(om.bgr_rows(r["rgb64"]), r["bgr"]), key
    r = renders["A", 1, 0]
    padded = om.bgr_rows(r["rgb64"], 3 * ts.WIDTH + 8)
    assert np.array_equal(padded[:, :3 * ts.WIDTH], r["bgr"]) and (padded[:, 3 * ts.WIDTH:] == 0).all()


def test_background_scenes_deliver_their_triples():
    t = om.threshold_values()
    seen = set()
    for spec in ts.background_scenes():
        for spp in (1, 2, 3):
            spec.antialias = spp
            r = ref64.render(spec)
            bg = (r["rgb64"] == r["rgb64"][0, 0]).all(axis=2)
            assert bg.sum() >= 100 and (~bg).sum() >= 4
            if spp < 3:            # (v + v + v) / 3 need not be v
                assert np.array_equal(r["rgb64"][0, 0], np.array(spec.background))
            assert om.same_f32(om.to_f32(r["rgb64"]), r["rgb32"]).all() and np.array_equal(om.bgr_rows(r["rgb64"]), r["bgr"])
        seen |= set(np.array(spec.background).view(np.uint64).tolist())
    assert {int(x) for x in t[[0, 254]].view(np.uint64).reshape(-1)} <= seen
