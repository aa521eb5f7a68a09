"""How far a last-ulp difference in cos / sin / pow can move the trig scenes'
images, measured on the oracle alone (ref_opts.trig_ulps; tests/trig_scenes.py).

The device tests (test_gpu_path.py assert_trig_exact) hold the path kernel to
every BGR byte that no perturbation moves.  That is only a tight check if nearly
all bytes are such: here every trig scene is required to keep its ray counts and
NaN mask under every perturbation and to have >= 99.99% stable bytes.  The cap is
a condition on the choice of scene and seed, not a measurement: a new scene that
misses it gets another seed or geometry.
"""
import numpy as np
import pytest

from oracle import ref64
import trig_scenes
from trig_scenes import TRIG_SCENES, PERTURBATIONS, envelope


def test_perturbation_set():
    assert PERTURBATIONS[0] == (0, False)
    assert set(PERTURBATIONS[1:]) == {(1, False), (-1, False), (4, False), (-4, False), (1, True), (-1, True)}
    assert trig_scenes.STABLE_MIN == 0.9999


@pytest.mark.parametrize("name", sorted(TRIG_SCENES))
def test_trig_scene_is_stable_under_ulp_perturbation(name):
    build, seed, jitter = TRIG_SCENES[name]
    spec = build()
    env = envelope(spec, seed, jitter)
    print(f"{name}: stable share {env.stable_share:.6f}, largest relative f64 change {env.max_rel:.3g}, "
          f"rays {env.ref['counts']['rays']}, NaN components {int(env.nan.sum())}")
    for (k, h), r in zip(PERTURBATIONS, env.renders):
        assert r["counts"]["rays"] == env.ref["counts"]["rays"], (k, h)
        assert r["counts"]["shadow_rays"] == env.ref["counts"]["shadow_rays"], (k, h)
        assert np.array_equal(np.isnan(r["rgb64"]), env.nan), (k, h)
    assert env.stable_share >= trig_scenes.STABLE_MIN
    env.check_scene()


def test_the_knob_perturbs_and_is_a_pure_function_of_the_call():
    """The knob does move the f64 colours (so an all-stable image is a finding about
    the scene, not a dead knob); hashed mode mixes both directions; and a render does
    not depend on the thread count or the tile it is part of."""
    build, seed, jitter = TRIG_SCENES["stochastic_dof"]
    spec = build()
    env = envelope(spec, seed, jitter)
    base = env.ref["rgb64"]
    by = dict(zip(PERTURBATIONS, env.renders))
    for key in PERTURBATIONS[1:]:
        assert not np.array_equal(by[key]["rgb64"], base), key
    assert 0.0 < env.max_rel < 1e-9          # a few ulp of f64, far below the f32 tolerance of the device tests
    up, dn, hs = by[(1, False)]["rgb64"], by[(-1, False)]["rgb64"], by[(1, True)]["rgb64"]
    assert not np.array_equal(hs, up) and not np.array_equal(hs, dn)
    one = ref64.render(spec, jitter=jitter, seed=seed, rng=1, trig_ulps=1, trig_hashed=True, threads=1)
    assert np.array_equal(one["rgb64"], hs, equal_nan=True)
    tile = ref64.render(spec, jitter=jitter, seed=seed, rng=1, trig_ulps=1, trig_hashed=True, x0=7, tile_w=20,
                        y0=5, tile_h=11)
    assert np.array_equal(tile["rgb64"], hs[5:16, 7:27], equal_nan=True)


def test_srgb_tables_are_not_perturbed():
    """to_srgb's thresholds come from pow too (color.rs tables); the knob leaves them
    alone: a centre-jitter Phong image changes only through its specular pow."""
    before = ref64.srgb_tables()
    build, seed, jitter = TRIG_SCENES["dof_config2"]
    ref64.render(build(), jitter=jitter, seed=seed, rng=1, trig_ulps=4)
    assert ref64.srgb_tables() == before
