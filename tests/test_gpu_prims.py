"""The sphere test, the plane test and the shading arithmetic on the device, record by record
(rt_isect_check, rt_shade_check: probes.hip calls the functions of trace_prims.hpp and trace_shade.hpp that the render kernels
call), bit for bit against prim_model.py, which test_prim_model.py pins to the oracle on the CPU; and the
device's pow, sin and cos, measured against the host libm and against correctly rounded values
(tests/golden/libm_cr.npz).  DESIGN.md §4 "Primitive probes".

One launch per probe, shared by the tests of this module: 1.74 * 10^6 intersection records, 10^6 shading
records, fixed seeds."""
import os

import numpy as np
import pytest

import prim_model as pm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENVELOPE = 4            # the project's own libm envelope: the largest k of test_oracle_trig.py
# The device's largest distance from the correctly rounded fixture, as measured on an MI355X (ROCm 7.2's OCML),
# in whole representable values: there is no noise to allow for, so the test allows nothing above it.
DEVICE_CR_MAX = {"pow": 1, "sin": 1, "cos": 1}


def _mismatch(ok, lab):
    bad = ~ok
    names, counts = np.unique(lab[bad], return_counts=True)
    return f"{bad.sum()} records differ, by class {dict(zip(names.tolist(), counts.tolist()))}, first {np.flatnonzero(bad)[:5].tolist()}"


@pytest.fixture(scope="module")
def isect(gpu_ctx):
    rays, sph, pl, lab = pm.isect_records()
    cov, m, p = pm.coverage(rays, sph, pl, lab)
    return {"out": gpu_ctx.isect_check(rays, sph, pl), "sphere": m, "plane": p, "lab": lab, "cov": cov}


def test_records_sit_on_the_decisions(isect):
    """The coverage conditions, from the model's intermediates alone: >= 10^4 hits, misses and second-root
    answers; >= 500 records with disc == 0 (on the integer lattices alone); >= 10^3 on each side of each edge of
    div_k's window of 2a (biased exponent 920-922 | 923-926 and 1120-1123 | 1124-1126); >= 10^3 hits whose
    positive numerator is outside the numerator window -- through a 2a outside its window, which leaves no
    numerator window at all, and >= 10^3 hits each with 2a below 2^-1020 and above 2^1019, where the reciprocal is
    no normal number and the three correction operations alone answer wrongly; >= 100 records per plane special
    (0/0, x/0 of either sign, t = +0 and -0, normals 1e-35 and 1e34 long, inf - inf).  The numerator window's own
    ends (2^-900, 2^600) are not hunted: with a finite nonzero discriminant |x| stays between about 2^-590 and
    2^513, so no finite numerator reaches them."""
    for k, floor in pm.COVERAGE_FLOOR.items():
        assert isect["cov"][k] >= floor, (k, isect["cov"][k], floor)


@pytest.mark.parametrize("form", ["bf", "br"])
def test_sphere_test_is_the_model_bit_for_bit(isect, form):
    """sphere_t<true> (bf: the branch-free form of every LDS and BVH walk, with its own restatement of the
    division's correction steps and window test) and sphere_t<false> (br: the branchy form of the binary16
    walk): the verdict, t, the hit point o + d t and hit_normal, each bit for bit the model's."""
    out, m, lab = isect["out"], isect["sphere"], isect["lab"]
    ok = out["hit_" + form] == m["hit"]
    assert ok.all(), "verdict: " + _mismatch(ok, lab)
    for name, got, want in (("t", out["t_" + form][:, None], m["t"][:, None]), ("point", out["pt_" + form], m["pt"]),
                            ("normal", out["n_" + form], m["n"])):
        ok = pm.bits_equal(got, want).all(axis=1)
        assert ok.all(), name + ": " + _mismatch(ok, lab)


def test_sphere_forms_agree_with_each_other(isect):
    out = isect["out"]
    ok = out["hit_bf"] == out["hit_br"]
    for k in ("t", "pt", "n"):
        a, b = out[k + "_bf"], out[k + "_br"]
        ok &= pm.bits_equal(a.reshape(len(ok), -1), b.reshape(len(ok), -1)).all(axis=1)
    assert ok.all(), _mismatch(ok, isect["lab"])


def test_plane_test_is_the_model_bit_for_bit(isect):
    """plane_t's t (NaN, +-inf and +-0 included) and its verdict `not t <= 0`."""
    out, p, lab = isect["out"], isect["plane"], isect["lab"]
    ok = pm.bits_equal(out["t_pl"], p["t"])
    assert ok.all(), "t: " + _mismatch(ok, lab)
    ok = out["hit_pl"] == p["hit"]
    assert ok.all(), "verdict: " + _mismatch(ok, lab)


# ---- shading and libm: one launch --------------------------------------------------------------------------
def _libm_columns(m):
    """pow (x, y) and trig x for m records: the fixture's operands first, then the Annex F specials of pow,
    then more operands of the same recipe, these without the fixture's restriction to normal results."""
    n = pm.N_FIXTURE
    c, y = pm.pow_operands(m, salt=11, normal_results=False)
    x = pm.trig_operands(m, salt=12)
    c[:n], y[:n] = pm.pow_operands(n)
    x[:n] = pm.trig_operands(n)
    sx, sy = np.meshgrid(pm.POW_SPECIAL_X, pm.POW_SPECIAL_Y, indexing="ij")
    k = sx.size
    c[n:n + k], y[n:n + k] = sx.ravel(), sy.ravel()
    special = np.zeros(m, bool)
    special[n:n + k] = True
    return c, y, x, special


@pytest.fixture(scope="module")
def shaded(gpu_ctx):
    rec, kinds, lab = pm.shade_records()
    c, y, x, special = _libm_columns(len(rec))
    rec[:, 24], rec[:, 25], rec[:, 26] = c, y, x
    return {"out": gpu_ctx.shade_check(rec, kinds), "rec": rec, "kinds": kinds, "lab": lab, "special": special}


def _model(s, p=None):
    r, k = s["rec"], s["kinds"]
    return pm.shade(r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12], r[:, 12:15], r[:, 15], r[:, 16], k[:, 0], k[:, 1],
                    r[:, 17:20], r[:, 20:23], r[:, 23], p=p)


def test_shading_terms_are_the_model_bit_for_bit(shaded):
    """light_dir (direction, squared range, has_range), fresnel_factor, shading_flags (both flags and f),
    reflect_ray and the half vector's cosine c of add_light, bit for bit the model's: unit and off-unit normals,
    point lights 1e-3 .. 1e6 away, directional lights 1e-35 .. 1e34 long, a zero half vector (0/0), a light at
    the hit point, ior 1, 1.5, 1e-3 and 1e3, n.d = 0, +-1 and above 1, significances around and equal to
    kMinSignificance.  The colour add_light leaves is the model's own association order applied to the DEVICE's
    power p = pow(c, exponent): bit-equal too.  p itself is held to numpy's pow of the model's c and the record's
    exponent: equal where c is 0, 1 or NaN or the exponent is 0 (C Annex F), within the envelope elsewhere."""
    out, lab = shaded["out"], shaded["lab"]
    m = _model(shaded, p=out["p"])
    # the classes did what they were built for
    assert (np.isnan(m["c"]) & (lab == "zero_half")).sum() >= 10 ** 4
    assert ((m["nd"] == 0.0) & (lab == "nd_zero")).sum() >= 10 ** 4 and ((np.abs(m["nd"]) == 1.0) & (lab == "nd_one")).sum() >= 10 ** 4
    assert ((np.abs(m["nd"]) > 1.0) & (lab == "nd_above_one")).sum() >= 10 ** 4
    edge = lab == "sig_edge"
    assert (m["diffuse"] & edge).sum() >= 10 ** 4 and (~m["diffuse"] & edge).sum() >= 10 ** 4
    assert (shaded["rec"][edge, 23] == pm.K_MIN_SIGNIFICANCE).sum() >= 10 ** 3
    for flag in ("has_range", "diffuse", "specular"):
        ok = out[flag] == m[flag]
        assert ok.all(), flag + ": " + _mismatch(ok, lab)
    with np.errstate(all="ignore"):
        want_p = np.power(m["c"], shaded["rec"][:, 15])
    exact = np.isnan(m["c"]) | (m["c"] == 0.0) | (m["c"] == 1.0) | (shaded["rec"][:, 15] == 0.0)
    assert exact.sum() >= 10 ** 5 and (~exact).sum() >= 5 * 10 ** 5
    ok = np.where(exact, pm.bits_equal(out["p"], want_p),
                  np.abs(pm.ordinal(out["p"]) - pm.ordinal(want_p)) <= ENVELOPE)
    assert ok.all(), "p: " + _mismatch(ok, lab)
    for name in ("ldir", "r2", "fresnel", "f", "refl", "c", "col"):
        ok = pm.bits_equal(out[name].reshape(len(lab), -1), m[name].reshape(len(lab), -1)).all(axis=1)
        assert ok.all(), name + ": " + _mismatch(ok, lab)


def test_pow_specials_equal_the_hosts(shaded):
    """pow on {0, -0, 1, NaN, inf} x {0, -0, 1, NaN, inf, -1} (C Annex F; pow(NaN, 0) = 1 is what
    IndirectPhong's specular fold feeds its 0/0 into): the host's results bit for bit."""
    sp = shaded["special"]
    x, y = shaded["rec"][sp, 24], shaded["rec"][sp, 25]
    assert len(x) == 30
    with np.errstate(all="ignore"):
        want = np.power(x, y)
    got = shaded["out"]["pow"][sp]
    ok = pm.bits_equal(got, want)
    assert ok.all(), [(a, b, g, w) for a, b, g, w in zip(x[~ok], y[~ok], got[~ok], want[~ok])]


def _host(shaded):
    r = shaded["rec"]
    with np.errstate(all="ignore"):
        return {"pow": np.power(r[:, 24], r[:, 25]), "sin": np.sin(r[:, 26]), "cos": np.cos(r[:, 26])}


def test_libm_within_the_envelope_of_the_hosts(shaded):
    """The device's pow(c, y) (c over [0, 1 + 2^-50], dense near 0 and 1; y of 0, 1, 2, 8, 32, 50, 1000, 0.5,
    2.5, 1e-3; subnormal and zero powers included), sin(x) and cos(x) (x = u 2 pi, u = k 2^-53 of [0, 1), the multiples of pi / 4 among them)
    within 4 representable values of numpy's on 10^6 operands each; how many differ at all and the largest
    distance are printed (DESIGN.md §4 records them)."""
    host = _host(shaded)
    keep = ~shaded["special"]
    for fn in ("pow", "sin", "cos"):
        d = np.abs(pm.ordinal(shaded["out"][fn][keep]) - pm.ordinal(host[fn][keep]))
        print(f"device {fn} vs host: {np.count_nonzero(d)} of {d.size} differ, largest distance {d.max()}")
        assert d.max() <= ENVELOPE, (fn, int(d.max()), shaded["rec"][keep][np.argmax(d), 24:27])


def test_libm_distance_from_correctly_rounded(shaded):
    """Against tests/golden/libm_cr.npz (mpmath, 200 bits, rounded once to nearest even; 20,000 operands per
    function): the device's largest distance is the one measured when this test was written, never above the
    envelope; the host libm's is printed beside it."""
    z = np.load(os.path.join(GOLDEN, "libm_cr.npz"))
    n = int(z["n"])
    assert n == pm.N_FIXTURE
    host = _host(shaded)
    for fn in ("pow", "sin", "cos"):
        dev = shaded["out"][fn][:n]
        # within the envelope of the host in full, so the fixture's low ordinal bits give the distance
        assert np.abs(pm.ordinal(dev) - pm.ordinal(host[fn][:n])).max() <= ENVELOPE
        d_dev = np.abs(pm.low16_distance(dev, z[fn + "_low16"]))
        d_host = np.abs(pm.low16_distance(host[fn][:n], z[fn + "_low16"]))
        print(f"{fn} vs correctly rounded: device {np.count_nonzero(d_dev)} of {n} differ, largest distance {d_dev.max()}; "
              f"host {np.count_nonzero(d_host)} differ, largest distance {d_host.max()}")
        assert d_dev.max() <= ENVELOPE, fn
        assert d_dev.max() <= DEVICE_CR_MAX[fn], (fn, int(d_dev.max()))
