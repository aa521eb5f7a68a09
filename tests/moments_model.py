"""The rule of a moments accumulator (include/raytrace_amd.h, "second moments") in numpy,
operation by operation.  Every numpy operation below is one IEEE f64 operation on each element: numpy
does not fuse a product with the sum that follows it, so `Q + s * s` is two roundings, as the rule says.

accumulate  the sums S and the sums of squares Q of a stack of per-sample colours, one sample at a time in
            sample order; sample 0 stores 0.0 + s and 0.0 + s * s without reading what was there.
squares_first  the other order of the sum of squares (what the rule forbids), for the tests' sensitivity checks.
estimate    variance of the mean, relative error and the pixels above a threshold from S, Q and n >= 2.
"""
import numpy as np


def accumulate(samples, S0=None, Q0=None, first=0):
    """samples: float64 [k, h, w, 3], the colours of samples first .. first + k - 1.  S0, Q0: the sums of the
    samples before `first` (ignored when first is 0: sample 0 never reads).  -> (S, Q)."""
    samples = np.asarray(samples, np.float64)
    S = None if first == 0 or S0 is None else np.array(S0, np.float64)
    Q = None if first == 0 or Q0 is None else np.array(Q0, np.float64)
    if first != 0 and (S is None or Q is None):
        raise ValueError("samples after the first continue given sums")
    with np.errstate(all="ignore"):
        for k in range(samples.shape[0]):
            s = samples[k]
            q = s * s
            if first + k == 0:
                S = 0.0 + s
                Q = 0.0 + q
            else:
                S = S + s
                Q = Q + q
    if S is None:                       # no samples at all: BLACK
        S = np.zeros(samples.shape[1:], np.float64)
        Q = np.zeros(samples.shape[1:], np.float64)
    return S, Q


def squares_first(samples, split):
    """NOT the rule: the sum of squares a device would give that summed each call's squares among themselves
    first (split: the calls' sample counts) and added the partial sums afterwards.  The tests use it to show
    that their stacks and splits tell the two orders apart."""
    samples = np.asarray(samples, np.float64)
    total, at = None, 0
    with np.errstate(all="ignore"):
        for n in split:
            part = None
            for s in samples[at:at + n]:
                part = 0.0 + s * s if part is None else part + s * s
            total = part if total is None else total + part
            at += n
    return total


def estimate(S, Q, n, floor, threshold):
    """-> dict(v float64 [h, w, 3], err float64 [h, w], variance float32, error float32, above_mask bool [h, w],
    above int)."""
    if n < 2:
        raise ValueError("a variance needs at least 2 samples")
    S = np.asarray(S, np.float64)
    Q = np.asarray(Q, np.float64)
    N = np.float64(n)
    with np.errstate(all="ignore"):
        mean = S / N
        d = Q - (S * mean)
        den = N * (N - np.float64(1.0))
        v = np.where(d < 0.0, np.float64(0.0), d / den)          # a NaN d: d < 0 is false, NaN / den is NaN
        a = np.abs(mean)
        err = np.sqrt((v[..., 0] + v[..., 1]) + v[..., 2]) / (np.float64(floor) + ((a[..., 0] + a[..., 1]) + a[..., 2]))
        above_mask = ~(err <= np.float64(threshold))
        return dict(v=v, err=err, variance=v.astype(np.float32), error=err.astype(np.float32), above_mask=above_mask,
                    above=int(above_mask.sum()))
