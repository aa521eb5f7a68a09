"""The rule of a moments accumulator (include/raytrace_amd.h, "second moments") without a GPU.

tests/moments_model.py states the rule in numpy; tests/test_gpu_moments.py demands the device's bits of it.
Here the model is checked against a scalar restatement in plain Python floats (IEEE f64, one operation per
operator) on stacks built to reach every branch of the rule, shown to be sensitive to the order of the sum of
squares, and tied to the oracle where all samples are equal; then the binding and the host-only checkpoint calls.
"""
import math
import struct

import numpy as np
import pytest

import libraytrace as lr
from libraytrace import scenes
from oracle import ref64
import moments_model as model

INF, NAN = float("inf"), float("nan")


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    """Bit for bit, any NaN equal to any NaN (IEEE leaves a NaN's payload open)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((u64(a) == u64(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the scalar restatement ----

def scalar_accumulate(stack, S0=None, Q0=None, first=0):
    k, h, w, _ = stack.shape
    S = np.zeros((h, w, 3)) if S0 is None else np.array(S0, np.float64)
    Q = np.zeros((h, w, 3)) if Q0 is None else np.array(Q0, np.float64)
    for y in range(h):
        for x in range(w):
            for c in range(3):
                s_run, q_run = float(S[y, x, c]), float(Q[y, x, c])
                for i in range(k):
                    s = float(stack[i, y, x, c])
                    q = s * s
                    if first + i == 0:
                        s_run, q_run = 0.0 + s, 0.0 + q
                    else:
                        s_run, q_run = s_run + s, q_run + q
                S[y, x, c], Q[y, x, c] = s_run, q_run
    return S, Q


def scalar_estimate(S, Q, n, floor, threshold):
    h, w, _ = S.shape
    v = np.zeros((h, w, 3))
    err = np.zeros((h, w))
    above = 0
    N = float(n)
    for y in range(h):
        for x in range(w):
            mean = [float(S[y, x, c]) / N for c in range(3)]
            for c in range(3):
                d = float(Q[y, x, c]) - (float(S[y, x, c]) * mean[c])
                v[y, x, c] = 0.0 if d < 0.0 else d / (N * (N - 1.0))
            tot = (float(v[y, x, 0]) + float(v[y, x, 1])) + float(v[y, x, 2])
            root = tot if math.isnan(tot) else math.sqrt(tot)
            e = root / (floor + ((abs(mean[0]) + abs(mean[1])) + abs(mean[2])))
            err[y, x] = e
            above += 0 if e <= threshold else 1
    return v, err, above


def stacks():
    rng = np.random.default_rng(20261021)
    out = {"random": rng.standard_normal((7, 3, 5, 3)) * np.exp(rng.uniform(-8, 8, (7, 3, 5, 3)))}
    big = 2.0 ** 100
    cancel = np.full((6, 2, 2, 3), 0.25)
    cancel[0], cancel[1] = big, -big                  # S cancels to the small samples, Q stays near 2 * 2^200
    cancel[3, 0, 0], cancel[4, 0, 0] = -big, big
    out["cancelling"] = cancel
    special = rng.uniform(0.0, 1.0, (4, 2, 3, 3))
    special[0, 0, 0] = -0.0                           # a first sample of -0.0: 0.0 + s is +0.0
    special[:, 0, 1] = -0.0
    special[1, 0, 2] = NAN
    special[2, 1, 0] = INF
    special[1, 1, 1, 0], special[2, 1, 1, 0] = INF, -INF    # S: inf - inf = NaN, Q: inf
    special[0, 1, 2] = 1e200                          # the square overflows
    special[3, 1, 2, 1] = -1e200
    out["special"] = special
    tiny = np.full((3, 1, 2, 3), 1e-160)              # the square is denormal (1e-320)
    tiny[1, 0, 1] = 3e-162                            # ... or underflows to 0
    out["denormal_squares"] = tiny
    return out


@pytest.mark.parametrize("name", ["random", "cancelling", "special", "denormal_squares"])
def test_model_against_the_scalar_loop(name):
    stack = stacks()[name]
    S, Q = model.accumulate(stack)
    S1, Q1 = scalar_accumulate(stack)
    assert same_bits(S, S1) and same_bits(Q, Q1)
    # continued from given sums: any split is the one-shot stack
    for k in range(1, stack.shape[0]):
        Sa, Qa = model.accumulate(stack[:k])
        Sb, Qb = model.accumulate(stack[k:], Sa, Qa, first=k)
        assert same_bits(Sb, S) and same_bits(Qb, Q)
        Sc, Qc = scalar_accumulate(stack[k:], Sa, Qa, first=k)
        assert same_bits(Sc, S) and same_bits(Qc, Q)
    n = stack.shape[0]
    for floor, thr in ((1e-3, 0.05), (1.0, 1e-9), (1e-300, 1e300)):
        est = model.estimate(S, Q, n, floor, thr)
        v, err, above = scalar_estimate(S, Q, n, floor, thr)
        assert same_bits(est["v"], v) and same_bits(est["err"], err) and est["above"] == above
        assert est["variance"].dtype == np.float32 and est["error"].dtype == np.float32
    if name == "cancelling":
        assert np.all(np.abs(S) < 8.0) and np.all(Q >= 2.0 ** 200)
    if name == "special":
        assert not np.signbit(S[0, 1]).any() and np.isnan(S[1, 1, 0]) and Q[1, 1, 0] == INF and Q[1, 2, 0] == INF
        est = model.estimate(S, Q, n, 1e-3, 0.05)
        assert np.isnan(est["err"][1, 1]) and est["above_mask"][1, 1]           # a NaN err is above
    if name == "denormal_squares":
        assert 0.0 < Q[0, 0, 0] < 2.3e-308 and Q[0, 0, 0] == 3 * 1e-320


def test_sample_zero_never_reads():
    stack = stacks()["random"]
    junk = np.full(stack.shape[1:], NAN)
    S, Q = model.accumulate(stack, junk, junk, first=0)
    S1, Q1 = model.accumulate(stack)
    assert same_bits(S, S1) and same_bits(Q, Q1) and not np.isnan(Q).any()


def test_negative_d_clamps_and_nan_d_stays():
    n = 3
    s = 0.7
    S = np.full((1, 4, 3), 3 * s)
    mean = S / 3.0
    prod = S * mean
    Q = prod.copy()
    Q[0, 0] = np.nextafter(prod[0, 0], -INF)          # d one step below 0: clamps to 0.0
    Q[0, 1] = np.nextafter(prod[0, 1], INF)           # d one step above 0: stays
    S[0, 2], Q[0, 2] = INF, INF                       # mean inf, S * mean inf, inf - inf: d is NaN
    S[0, 3, 1], Q[0, 3, 1] = NAN, 1.0
    est = model.estimate(S, Q, n, 1e-3, 0.05)
    d00 = float(Q[0, 0, 0]) - float(S[0, 0, 0]) * (float(S[0, 0, 0]) / 3.0)
    assert d00 < 0.0
    assert (est["v"][0, 0] == 0.0).all() and not np.signbit(est["v"][0, 0]).any() and est["err"][0, 0] == 0.0
    assert (est["v"][0, 1] > 0.0).all()
    assert np.isnan(est["v"][0, 2]).all() and np.isnan(est["err"][0, 2]) and est["above_mask"][0, 2]
    assert np.isnan(est["v"][0, 3, 1]) and est["v"][0, 3, 0] == 0.0 and est["above_mask"][0, 3]
    assert not est["above_mask"][0, 0] and est["above"] == int(est["above_mask"].sum())
    v, err, above = scalar_estimate(S, Q, n, 1e-3, 0.05)
    assert same_bits(est["v"], v) and same_bits(est["err"], err) and est["above"] == above


def test_threshold_is_compared_on_the_f64_value():
    stack = stacks()["random"]
    S, Q = model.accumulate(stack)
    n = stack.shape[0]
    err = model.estimate(S, Q, n, 1e-3, 1.0)["err"]
    e = float(err[1, 2])
    assert e > 0.0 and math.isfinite(e)
    at = model.estimate(S, Q, n, 1e-3, e)
    assert not at["above_mask"][1, 2]                                   # err == threshold: not above
    below = model.estimate(S, Q, n, 1e-3, float(np.nextafter(e, 0.0)))
    assert below["above_mask"][1, 2]                                    # err one representable value higher: above
    # the f32 image cannot decide this: both thresholds round to the same float
    assert np.float32(e) == np.float32(np.nextafter(e, 0.0))
    assert at["above"] + 1 == below["above"] or (err == e).sum() > 1


squares_first = model.squares_first


def test_the_order_of_the_squares_shows_in_the_bits():
    """1, then three times 2^-27: by the rule every 2^-54 is rounded away from 1 + 2^-54, one at a time, and Q
    is 1; summed among themselves first the three are 3 * 2^-54, and 1 + 3 * 2^-54 rounds up to 1 + 2^-52.  So a
    device that summed a call's squares first would fail the split tests."""
    a = 2.0 ** -27
    stack = np.empty((4, 1, 1, 3))
    stack[0], stack[1:] = 1.0, a
    S, Q = model.accumulate(stack)
    assert (Q == 1.0).all()
    other = squares_first(stack, (1, 3))
    assert (other == 1.0 + 2.0 ** -52).all() and not same_bits(other, Q)
    assert same_bits(squares_first(stack, (1, 1, 1, 1)), Q)
    # ... and on colours of an ordinary render's kind (values in [0, 1) with full mantissas), for the GPU test's
    # splits: the rounding of every partial sum depends on the order.  (The cancelling scene does not show this
    # for Q: its squares are 2^200 and a few small powers of two, which add exactly or vanish in any order; the
    # GPU test therefore asserts the same on the very stack it compares with.)
    rng = np.random.default_rng(5)
    stack = rng.uniform(0.0, 1.0, (9, 32, 48, 3))
    Q = model.accumulate(stack)[1]
    for split in ((1, 8), (4, 5), (1, 1, 7), (2, 3, 4)):
        differ = int((u64(squares_first(stack, split)) != u64(Q)).sum())
        print(f"split {split}: {differ} of {Q.size} squares differ")
        assert differ >= Q.size // 20, (split, differ)


# ---- tie to the oracle ----

def test_equal_samples_tie_the_model_to_the_oracle():
    """Centre jitter: every sample is the spp = 1 render's colour, so the model's S over n copies must be the
    oracle's spp = n image times n (a division by a power of two and back is exact away from the denormals)."""
    spec = scenes.config3(48, 32, n=60)
    spec.antialias = 1
    s0 = ref64.render(spec)["rgb64"]
    assert np.isfinite(s0).all() and (s0 != 0.0).any()
    for n in (2, 4, 8):
        spec.antialias = n
        ref = ref64.render(spec)["rgb64"]
        nz = ref[ref != 0.0]
        assert (np.abs(nz) >= 2.3e-308).all() and (np.abs(nz) * n < 1e308).all(), "a denormal: the tie is not exact"
        S, Q = model.accumulate(np.stack([s0] * n))
        assert same_bits(S, ref * float(n))
        # constant pixels: Q and S * mean each carry at most about (n + 1) roundings of relative size 2^-53 on
        # n s^2, so d <= (2n + 3) 2^-53 n s^2, and v = d / (n (n - 1)) <= 7 * 2^-53 s^2 since (2n + 3) / (n - 1) <= 7
        est = model.estimate(S, Q, n, 1e-3, 0.05)
        mean = S / float(n)
        assert (est["v"] >= 0.0).all() and (est["v"] <= 8.0 * 2.0 ** -53 * mean * mean).all()


# ---- the binding and the host-only calls ----

def test_symbols_and_abi():
    assert lr.RT_ABI_VERSION == 10 and lr.lib.rt_abi_version() == 10
    for name in ("rt_accum_create_moments", "rt_accum_has_moments", "rt_accum_download_moments", "rt_accum_upload_moments",
                 "rt_accum_noise", "rt_accum_noise_host", "rt_checkpoint_write_moments", "rt_checkpoint_read_moments"):
        assert hasattr(lr.lib, name), name
        assert name in lr.header_functions(), name
    for name in ("has_moments", "download_moments", "upload_moments", "noise", "noise_device"):
        assert hasattr(lr.Accumulator, name), name
    assert len(lr.KERNEL_FAMILIES) == 8                                 # RT_KF_COUNT: accum_noise is timed as compose


def test_checkpoint_version_2_round_trip_and_refusals(tmp_path):
    o = lr.render_opts(40, 30, max_depth=4, spp=1, jitter=lr.RT_JITTER_RANDOM, seed=77, x0=3, tile_w=7, y0=2, tile_h=5)
    rng = np.random.default_rng(3)
    sums = rng.standard_normal((5, 7, 3))
    sq = rng.uniform(0, 9, (5, 7, 3))
    sums[0, 0, 0], sq[0, 0, 1], sq[4, 6, 2] = -0.0, INF, 5e-324
    p2, p1 = tmp_path / "m.ckpt", tmp_path / "p.ckpt"
    lr.checkpoint_write_moments(p2, o, 0xABCDEF, 6, sums, sq)
    assert p2.stat().st_size == 88 + 48 * 35
    assert struct.unpack("<8sI", p2.read_bytes()[:12]) == (b"RTAMDCKP", 2)
    ro, h, n, s, q = lr.checkpoint_read_moments(p2)
    assert (h, n, ro.tile_w, ro.tile_h, ro.seed, ro.x0) == (0xABCDEF, 6, 7, 5, 77, 3)
    assert np.array_equal(u64(s), u64(sums)) and np.array_equal(u64(q), u64(sq))
    assert lr.checkpoint_read_moments(p2, header_only=True)[2:] == (6, None, None)
    # each reader refuses the other's file
    with pytest.raises(lr.RtError) as e:
        lr.checkpoint_read(p2)
    assert e.value.code == lr.RT_E_INVALID
    lr.checkpoint_write(p1, o, 0xABCDEF, 6, sums)
    assert p1.stat().st_size == 88 + 24 * 35
    with pytest.raises(lr.RtError) as e:
        lr.checkpoint_read_moments(p1)
    assert e.value.code == lr.RT_E_INVALID
    assert np.array_equal(u64(lr.checkpoint_read(p1)[3]), u64(sums))
    # the writer: sizes that are not the tile's
    with pytest.raises(lr.RtError) as e:
        lr.checkpoint_write_moments(tmp_path / "x.ckpt", o, 1, 1, sums[:4], sq[:4])
    assert e.value.code == lr.RT_E_INVALID and not (tmp_path / "x.ckpt").exists()
    # a version 2 file cut inside the squares
    cut = tmp_path / "cut.ckpt"
    cut.write_bytes(p2.read_bytes()[:88 + 24 * 35 + 16])
    for header_only in (True, False):
        with pytest.raises(lr.RtError) as e:
            lr.checkpoint_read_moments(cut, header_only=header_only)
        assert e.value.code == lr.RT_E_INVALID
