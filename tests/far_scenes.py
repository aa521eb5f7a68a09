"""Scenes whose rays start far from the spheres, compared with the spheres' extent E
("the far-origin rule"): the reference's f64 quadratic (shapes.rs:60-88)
cancels in |oc|^2 - r^2 and in b^2 - 4a cc, so from |oc| away it reports hits up to about
4 sqrt(2^-53) |oc| outside a small sphere, far outside the sphere's padded box.  Shared by
test_lightgrid.py (the grids' host mirrors), test_gpu_culling.py (the slab test on the
device) and test_gpu_parity.py (whole frames)."""
import numpy as np

from libraytrace import scenes

PAD = 1e-5                 # the box padding is PAD * (1 + E) (rt_scene_upload.cpp)
_M = scenes.phong((0.6, 0.5, 0.4), (0.4, 0.4, 0.4), 20.0, (0.02, 0.02, 0.02))


def extent(c, r):
    """E: the largest |centre +- radius| over the spheres (arrays [n, 3], [n])."""
    return float(np.max(np.abs(np.concatenate([c - r[:, None], c + r[:, None]]))))


def telephoto(D, n=40, size=64):
    """A camera D away from n tiny spheres (centres within +-2e-3, radii 1e-5..1e-4, so E is
    about 2e-3), its frame just covering them."""
    s = scenes.SceneSpec(width=size, height=size, max_depth=3, background=(0.05, 0.1, 0.2), name="telephoto",
                         camera={"ctor": "new", "position": (0.0, 0.0, D), "look": (0.0, 0.0, -1.0),
                                 "up": (0.0, 1.0, 0.0), "im_dist": D / 2e-3})
    rng = scenes.SplitMix64(3)
    for _ in range(n):
        x, y, z = rng.uniform(-2e-3, 2e-3), rng.uniform(-2e-3, 2e-3), rng.uniform(-2e-3, 2e-3)
        s.sphere((x, y, z), 10 ** rng.uniform(-5, -4), _M)
    s.point_light((0.5, 1.0, 2.0), (0.9, 0.9, 0.9))
    return s


def floor(Z, n=40, size=64):
    """n tiny spheres around (0, 3, 1) one unit in front of a point light at (0, 3, 0), seen from
    the floor y = 0 around z = Z: a camera Z / 25 above the floor looks straight down on a
    square of half-width Z / 25, and every floor point's shadow ray passes the spheres from Z away."""
    H = Z / 25.0
    s = scenes.SceneSpec(width=size, height=size, max_depth=2, background=(0.05, 0.1, 0.2), name="floor",
                         camera={"ctor": "new", "position": (0.0, H, Z), "look": (0.0, -1.0, 0.0),
                                 "up": (0.0, 0.0, 1.0), "im_dist": 1.0})
    rng = scenes.SplitMix64(5)
    for _ in range(n):
        x, y, z = rng.uniform(-0.02, 0.02), 3.0 + rng.uniform(-0.02, 0.02), 1.0 + rng.uniform(-0.02, 0.02)
        s.sphere((x, y, z), 10 ** rng.uniform(-5, -4), _M)
    s.plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), scenes.phong((0.7, 0.7, 0.7), (0.0, 0.0, 0.0), 1.0, (0.05, 0.05, 0.05)))
    # (n . l is 3 / Z on that floor: a light bright enough for its diffuse term to reach the bytes)
    s.point_light((0.0, 3.0, 0.0), (0.3 * Z, 0.3 * Z, 0.3 * Z))
    return s


def cloud(E, n, seed, rlo=1e-5, rhi=1e-3):
    """n spheres with centres uniform in [-E, E]^3 and radii log-uniform in [rlo, rhi] (1 + E)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-E, E, (n, 3))
    r = (1.0 + E) * 10 ** rng.uniform(np.log10(rlo), np.log10(rhi), n)
    return c, r


def cloud_spec(c, r, camera, lights=()):
    s = scenes.SceneSpec(width=64, height=64, max_depth=1, camera=dict(camera), name="cloud")
    for ck, rk in zip(c.tolist(), r.tolist()):
        s.sphere(tuple(ck), rk, _M)
    for L in lights:
        s.point_light(tuple(L), (1.0, 1.0, 1.0))
    return s


def phantom_radius(r, dist):
    """How far from the centre a ray from `dist` away can pass and still be reported as a hit:
    |disc error| <= 64 * 2^-53 * a * |oc|^2 against disc = 4a (r^2 - p^2)."""
    return np.sqrt(r * r + 16.0 * 2.0 ** -53 * dist * dist)


def aim(rng, o, c, r, k, offset):
    """Unit directions from the points o [m, 3] that pass sphere k[m] at `offset` [m] (absolute)
    from its centre, in a random direction perpendicular to the line of sight."""
    to = c[k] - o
    dist = np.linalg.norm(to, axis=1)
    w = to / dist[:, None]
    u = np.cross(w, rng.normal(size=w.shape))
    u /= np.linalg.norm(u, axis=1)[:, None]
    d = to + u * np.asarray(offset)[:, None]
    return d / np.linalg.norm(d, axis=1)[:, None]


def miss_distance(o, d, c):
    """Perpendicular distance of the centres c [n, 3] from the line o + t d (f64, |d| = 1)."""
    oc = c - o
    along = oc @ d
    return np.sqrt(np.maximum(np.einsum("ij,ij->i", oc, oc) - along * along, 0.0))
