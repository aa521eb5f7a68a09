"""The inputs of the GPU order test of progressive rendering, established from the oracle alone (no GPU).

tests/test_gpu_progressive.py splits the cancelling scene's samples over several rt_render_accumulate calls
and demands the oracle's f32 image bit for bit.  That only says something about the order of the sum across
the call boundary if another order -- each call's samples summed among themselves first, the partial sums
added afterwards -- gives another image for the splits it uses.  Here that is shown on the CPU: the oracle's
prefix renders spp = 1 .. n of the scene (ambient +-2^100 over a background of (0.25, 0.5, 0.75), seed 19)
give every sample's class (+2^100, -2^100 or background) from the net count rint(rgb64_k * k / 2^100); the
in-order sum of the recovered samples reproduces the oracle's spp = n image exactly; and the pixels where
"partial sums first" differs are counted.  Measured (red channel): (1,4) 30, (2,3) 17, (3,2) 16 pixels of
1536, (4,1) 0 (not used); spp 16 as (3,5,8): 4.  Required: at least 10 for the three splits of 5, at least 1
for (3,5,8).
"""
import numpy as np
import pytest

from libraytrace import scenes
from oracle import ref64

BIG = 2.0 ** 100
BACKGROUND = (0.25, 0.5, 0.75)
AMBIENT_SCALE = (1.0, 0.5, 0.25)       # the spheres' ambient colour is (a, 0.5 a, 0.25 a), a = +-2^100


def cancelling_spheres():
    """The scene of test_gpu_aa.py / test_gpu_path.py: unlit Phong spheres, ambient +2^100 and -2^100 in turn."""
    spec = scenes.SceneSpec(width=48, height=32, antialias=1, max_depth=2, camera=dict(scenes.DEFAULT_CAMERA),
                            background=BACKGROUND)
    n = 24
    for i in range(n):
        for j in range(n):
            a = BIG if (i + j) % 2 == 0 else -BIG
            spec.sphere((0.4 * (i - 0.5 * n), -0.2 + 0.4 * (j - 0.5 * n), -6.0), 0.18,
                        scenes.phong((0.0,) * 3, (0.0,) * 3, 1.0, (a, 0.5 * a, 0.25 * a)))
    return spec


_prefix = {}


def prefixes(n):
    """rgb64 of the oracle's spp = 1 .. n renders (jitter=1, rng=1, seed 19), each computed once."""
    spec = cancelling_spheres()
    for k in range(1, n + 1):
        if k not in _prefix:
            spec.antialias = k
            _prefix[k] = ref64.render(spec, jitter=1, seed=19, rng=1)["rgb64"]
    return [_prefix[k] for k in range(1, n + 1)]


def samples_of(n, channel):
    """[n, h, w] the value of every sample in `channel`, recovered from the prefix renders' net counts."""
    imgs = prefixes(n)
    net = [np.zeros_like(imgs[0][..., 0])]
    for k, img in enumerate(imgs, start=1):
        net.append(np.rint(img[..., channel] * k / (BIG * AMBIENT_SCALE[channel])))
    cls = np.stack([net[k] - net[k - 1] for k in range(1, n + 1)])
    assert np.isin(cls, (-1.0, 0.0, 1.0)).all()
    return np.where(cls == 0.0, BACKGROUND[channel], cls * (BIG * AMBIENT_SCALE[channel]))


def in_order(samples):
    acc = np.zeros_like(samples[0])
    for s in samples:                       # acc = 0.0; acc = acc + s_a
        acc = acc + s
    return acc


def partial_sums_first(samples, split):
    assert sum(split) == len(samples)
    total, at = None, 0
    for n in split:
        part = in_order(samples[at:at + n])
        total = part if total is None else total + part
        at += n
    return total


@pytest.mark.parametrize("channel", [0, 1, 2])
def test_in_order_sum_reproduces_the_oracle(channel):
    for n in (5, 16):
        s = samples_of(n, channel)
        assert np.array_equal(in_order(s) / float(n), prefixes(n)[n - 1][..., channel])
        # ... and every prefix on the way: a resolve after k samples is the spp = k render
        for k in range(1, n + 1):
            assert np.array_equal(in_order(s[:k]) / float(k), prefixes(n)[k - 1][..., channel])


@pytest.mark.parametrize("split,n,at_least", [((1, 4), 5, 10), ((2, 3), 5, 10), ((3, 2), 5, 10), ((3, 5, 8), 16, 1)],
                         ids=["1+4", "2+3", "3+2", "3+5+8"])
def test_partial_sums_first_is_another_image(split, n, at_least):
    s = samples_of(n, 0)
    want = in_order(s)
    other = partial_sums_first(s, split)
    differ = int((other != want).sum())
    print(f"split {split}: {differ} of {want.size} pixels differ (red channel)")
    assert differ >= at_least, differ
    # the difference survives the division and the rounding to f32: the GPU test compares f32 bits
    with np.errstate(over="ignore"):
        d32 = ((other / float(n)).astype(np.float32) != (want / float(n)).astype(np.float32)).sum()
    assert d32 >= at_least, d32


def test_the_split_that_shows_nothing_is_not_used():
    s = samples_of(5, 0)
    assert int((partial_sums_first(s, (4, 1)) != in_order(s)).sum()) == 0
