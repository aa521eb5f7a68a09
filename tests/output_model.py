"""The output stage restated in numpy -- a helper of test_output_model.py (which pins it on the CPU against
the oracle's and the host's to_srgb, an integer restatement of the f64 -> f32 rounding and ref_render's own
outputs) and of test_gpu_output.py (which holds the device's pixel writers to it, bit for bit) -- and the
operands both feed it.

The rule (main.rs:56-58, color.rs:593-600, 628-632): a pixel's f64 colour is its sum over the samples divided
by f64(samples); it is rounded ONCE to f32 (IEEE, to nearest, ties to even) for the f32 output, and each
channel is quantised FROM THE f64 VALUE, never from the f32, to the number of sRGB table entries <= it (NaN:
255); a BGR row is its pixels' b, g, r bytes followed by zero padding up to the pitch.  Every step below is
one numpy ufunc call: nothing is fused.
"""
import numpy as np

from oracle import ref64

TABLE = np.array(ref64.srgb_tables()[1], np.float64)      # the 255 thresholds T_0 < ... < T_254
assert TABLE.shape == (255,) and (np.diff(TABLE) > 0).all()

SAMPLES = (1, 2, 3, 7, 1000, 2 ** 31)                     # the divisors of the operand probe
NUDGES = (0, -1, 1, -2, 2)                                # sums around fl(v * n), in representable values
F32_MAX = float(np.finfo(np.float32).max)                 # 2^128 - 2^104
F32_OVERFLOW_TIE = 2.0 ** 128 - 2.0 ** 103                # halfway between F32_MAX and 2^128: ties to even = inf
F32_TINY = 2.0 ** -149                                    # the smallest f32 denormal
F32_MIN_NORMAL = 2.0 ** -126
CLASSES = ("tie_down", "tie_up", "denormal", "flush", "overflow", "neg_zero")


# ---- the rule ----------------------------------------------------------------------------------------
def quantise(v):
    """to_srgb: the number of table entries <= v (uint8); NaN gives 255."""
    v = np.asarray(v, np.float64)
    flat = v.reshape(-1)
    out = np.empty(flat.shape, np.uint8)
    for a in range(0, flat.size, 1 << 16):                # (bounded memory: 255 comparisons per value)
        x = flat[a:a + (1 << 16)]
        n = (TABLE[None, :] <= x[:, None]).sum(axis=1)
        out[a:a + (1 << 16)] = np.where(np.isnan(x), 255, n)
    return out.reshape(v.shape)


def binary_search(v, turns=8, guard=True, guard_ge=False):
    """The device's form of the quantiser (trace_types.hpp to_srgb) restated: the guard `!(v < T_254)` (or,
    guard_ge, the edit `v >= T_254`, which lets NaN through), then `turns` halvings of [0, 254].  For the CPU
    module: which edits of that function change its result at all."""
    v = np.asarray(v, np.float64).reshape(-1)
    lo, hi = np.zeros(v.shape, np.int64), np.full(v.shape, 254, np.int64)
    with np.errstate(invalid="ignore"):
        for _ in range(turns):
            mid = (lo + hi) >> 1
            lt = v < TABLE[mid]
            hi = np.where(lt, mid, hi)
            lo = np.where(lt, lo, mid + 1)
        if guard:
            lo = np.where((v >= TABLE[254]) if guard_ge else ~(v < TABLE[254]), 255, lo)
    return lo.astype(np.uint8)


def to_f32(v):
    """f64 -> f32, IEEE round to nearest, ties to even (numpy's cast; test_output_model.py holds it to
    to_f32_bits_integer)."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(v, np.float64).astype(np.float32)


def average(total, n):
    with np.errstate(all="ignore"):
        return np.asarray(total, np.float64) / np.float64(n)


def bgr_rows(rgb64, pitch=0):
    """[h, w, 3] f64 colours -> uint8 [h, pitch]: b, g, r per pixel, then zeros (main.rs:42)."""
    h, w, _ = rgb64.shape
    pitch = pitch or 3 * w
    assert pitch >= 3 * w
    out = np.zeros((h, pitch), np.uint8)
    out[:, :3 * w] = quantise(rgb64)[:, :, ::-1].reshape(h, 3 * w)
    return out


# ---- bit-level helpers -------------------------------------------------------------------------------
def f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_f32(a, b):
    """Bitwise equality of f32 arrays, NaN == NaN by position (payloads aside)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def ordinal(x):
    """float64 -> int64, monotone over the finite values and the infinities (+0 and -0 the same value): the
    distance between two values in representable values is the difference of their ordinals."""
    b = np.ascontiguousarray(x, np.float64).view(np.int64)
    return np.where(b < 0, np.int64(-2 ** 63) - b, b)


def step(x, k):
    """x moved by k representable values (k of either sign; x finite, not across an infinity)."""
    x = np.asarray(x, np.float64)
    o = ordinal(x.reshape(-1)) + np.int64(k)
    r = np.where(o < 0, np.int64(-2 ** 63) - o, o).astype(np.int64).view(np.float64)
    return float(r[0]) if x.ndim == 0 else r.reshape(x.shape)


def to_f32_bits_integer(v):
    """The f32 bit patterns of round-to-nearest-even(v) from v's own bits in integer arithmetic: the 53-bit
    significand shifted right to f32's grid (24 bits for a normal result, fewer below 2^-126), one guard bit
    and a sticky bit, a tie going to the even neighbour, the carry running into the exponent field.  NaN
    gives the canonical quiet NaN (NaNs are compared by position)."""
    b = np.ascontiguousarray(v, np.float64).view(np.uint64).reshape(-1)
    out = np.empty(b.shape, np.uint32)
    for i, x in enumerate(b.tolist()):
        sign, e, m = (x >> 63) << 31, (x >> 52) & 0x7FF, x & ((1 << 52) - 1)
        if e == 0x7FF:
            r = 0x7F800000 if m == 0 else 0x7FC00000
        elif e == 0:
            r = 0                                         # +-0 and the f64 denormals: far below 2^-150
        else:
            sig, E = m | (1 << 52), e - 1023              # the value is sig * 2^(E - 52)
            sh = 29 if E >= -126 else min(29 + (-126 - E), 63)
            q, guard, sticky = sig >> sh, (sig >> (sh - 1)) & 1, (sig & ((1 << (sh - 1)) - 1)) != 0
            q += 1 if guard and (sticky or (q & 1)) else 0
            r = ((E + 126) << 23) + q if E >= -126 else q  # (q carries 2^23: the hidden bit / the first normal)
            r = min(r, 0x7F800000)
        out[i] = sign | r
    return out.reshape(np.shape(v))


def f32_class(v):
    """{class: mask} of the f64 values v by what the rounding to f32 does with them (the classes of CLASSES)."""
    v = np.asarray(v, np.float64)
    r = to_f32(v)
    rb = f32_bits(r)
    fin = np.isfinite(v)
    back = r.astype(np.float64)
    with np.errstate(all="ignore"):
        lo32 = np.where(back <= v, r, np.nextafter(r, np.float32(-np.inf)))       # the f32 neighbours of v
        hi32 = np.where(back >= v, r, np.nextafter(r, np.float32(np.inf)))
        tie = fin & np.isfinite(lo32) & np.isfinite(hi32) & (lo32 != hi32) & \
            (v - lo32.astype(np.float64) == hi32.astype(np.float64) - v)
    tie |= fin & (np.abs(v) == F32_OVERFLOW_TIE)          # (its upper neighbour, 2^128, is no f32)
    went_out = np.abs(back) > np.abs(v)                   # the even neighbour is the one farther from zero
    return {"tie_down": tie & ~went_out, "tie_up": tie & went_out,
            "denormal": fin & (back != 0) & (np.abs(back) < F32_MIN_NORMAL),
            "flush": fin & (v != 0) & (back == 0),
            "overflow": fin & np.isinf(back),
            "neg_zero": rb == np.uint32(0x80000000)}


# ---- the operands ------------------------------------------------------------------------------------
def threshold_values():
    """The 510 values {T_i, nextbelow(T_i)}: [255, 2], column 0 the threshold."""
    return np.stack([TABLE, step(TABLE, -1)], axis=1)


def _f32_ties():
    """f64 values exactly halfway between two adjacent f32 values, over every f32 exponent (the denormal
    range and the overflow boundary included) and both parities of the lower neighbour."""
    lows = []
    for e in range(1, 255):                               # normal f32: one even and one odd mantissa per binade
        for mant in ((e * 0x9E3779) & 0x7FFFFE, ((e * 0x7F4A7C) & 0x7FFFFE) | 1, 0x7FFFFF if e % 2 else 0):
            lows.append((e << 23) | mant)
    k = np.unique(np.concatenate([np.arange(0, 40), 2 ** np.arange(3, 23), 2 ** np.arange(3, 23) - 1,
                                  (np.arange(1, 200) * 41957) % (1 << 23), [(1 << 23) - 2, (1 << 23) - 1]]))
    lows = np.concatenate([np.array(lows, np.uint32), k.astype(np.uint32)])       # ... and the denormal range
    lo = lows.view(np.float32).astype(np.float64)
    hi = (lows + np.uint32(1)).view(np.float32).astype(np.float64)
    hi[np.isinf(hi)] = 2.0 ** 128
    return (lo + hi) / 2.0                                # exact: 25 significant bits


def quotient_values():
    """The f64 values the probe aims a quotient at, by group: (values, labels)."""
    T = TABLE
    two = 2.0 ** -np.arange(1.0, 1075.0)                  # 2^-1 .. 2^-1074
    ties = _f32_ties()
    groups = {
        "threshold": T, "below": step(T, -1), "above": step(T, 1),
        "special": np.array([0.0, -0.0, -1.0, -T[0], -T[254], -1e-300, -1e300, np.inf, -np.inf, np.nan, 1.0,
                             step(1.0, -1), step(1.0, 1), 0.5, 2.0, 255.0, -np.nan,
                             *np.array([0x7FF0000000000001, 0xFFF8000000000123, 0x7FFFFFFFFFFFFFFF], np.uint64).view(np.float64)]),
        "under_t0": np.concatenate([T[0] * two[:1060], two[1020:], 3.0 * two[1024:]]),     # ... to the f64 denormals
        "tie": np.concatenate([ties, -ties]),
        "tie_below": np.concatenate([step(ties, -1), step(-ties, -1)]),
        "tie_above": np.concatenate([step(ties, 1), step(-ties, 1)]),
        "overflow": np.concatenate([s * np.concatenate([[F32_MAX, 2.0 ** 128, step(F32_MAX, 1), step(2.0 ** 128, -1)],
                                                         F32_OVERFLOW_TIE * 2.0 ** np.arange(1.0, 121.0)])
                                    for s in (1.0, -1.0)]),
        "flush": np.concatenate([s * np.concatenate([2.0 ** -150 * two[:120], 3.0 * 2.0 ** -152 * two[:40]])
                                 for s in (1.0, -1.0)]),
        "denormal": np.concatenate([s * np.concatenate([F32_TINY * np.arange(1.0, 41.0), 1.3e-39 * two[:20],
                                                         F32_TINY * (2.0 ** np.arange(1.0, 24.0) - 0.25)])
                                    for s in (1.0, -1.0)]),
    }
    vals = np.concatenate([np.asarray(g, np.float64) for g in groups.values()])
    labels = np.concatenate([np.full(len(g), name) for name, g in groups.items()])
    return vals, labels


def sum_values():
    """Sums that are operands in their own right, whatever the divisor: around DBL_MAX, the f64 denormals
    (denormal quotients under any divisor) and tiny sums whose quotient by 2^31 is a denormal."""
    big = np.finfo(np.float64).max
    tiny = 2.0 ** -1074
    s = np.concatenate([[big, step(big, -1), step(big, -2), big / 2, step(big / 2, 1), big / 3, big / 1000, 2.0 ** 1023],
                        tiny * np.arange(1.0, 33.0), tiny * (2.0 ** np.arange(5.0, 53.0) + 1.0),
                        2.0 ** -1022 * (1.0 + 2.0 ** -np.arange(1.0, 53.0)),
                        2.0 ** -1043 * np.arange(1.0, 64.0, 2.0), 2.0 ** -1022 * 2.0 ** np.arange(1.0, 32.0) * (1.0 + 2.0 ** -52)])
    return np.concatenate([s, -s])


def probe_sums(n):
    """The probe's sums for divisor n: (sums [m], target [m], label [m]).  target: the value of
    quotient_values() the sum aims at (NaN for a sum of sum_values()).  For n a power of two v * n is exact
    (asserted), so the quotient IS the target; for any other n the sums are fl(v * n) and the two values
    either side of it, and the model says where each quotient lands."""
    v, lab = quotient_values()
    with np.errstate(all="ignore"):
        p = v * np.float64(n)
        if n & (n - 1) == 0:
            ok = np.isfinite(p) | ~np.isfinite(v)
            back = p / np.float64(n)
            assert ((back == v) | np.isnan(v) | ~ok).all()
            sums, tgt, labs = [p[ok]], [v[ok]], [lab[ok]]
        else:
            ok = np.isfinite(p)
            sums = [step(p[ok], k) for k in NUDGES] + [p[~ok]]
            tgt = [v[ok]] * len(NUDGES) + [v[~ok]]
            labs = [lab[ok]] * len(NUDGES) + [lab[~ok]]
    extra = sum_values()
    sums.append(extra)
    tgt.append(np.full(extra.shape, np.nan))
    labs.append(np.full(extra.shape, "sum"))
    return np.concatenate(sums), np.concatenate(tgt), np.concatenate(labs)


def probe_tile(sums, width):
    """The sums laid out as a tile [rows, width, 3] of running sums (the last row padded with 0.25, so
    that every byte of the tile is an operand's or known) and the number of operands."""
    per = 3 * width
    rows = -(-sums.size // per)
    tile = np.full(rows * per, 0.25)
    tile[:sums.size] = sums
    return tile.reshape(rows, width, 3), sums.size


def threshold_coverage(sums, n):
    """[255, 2] bool: for threshold i, whether byte i and byte i + 1 occur among the quotients sums / n that
    are within two representable values of T_i."""
    q = average(sums, n)
    fin = np.isfinite(q)
    o, byte = ordinal(q[fin]), quantise(q[fin])
    ot = ordinal(TABLE)
    near = np.abs(o[None, :] - ot[:, None]) <= 2
    i = np.arange(255)[:, None]
    return np.stack([(near & (byte[None, :] == i)).any(axis=1), (near & (byte[None, :] == i + 1)).any(axis=1)], axis=1)
