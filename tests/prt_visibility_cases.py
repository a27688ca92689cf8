"""The scenes, points and direction sets of tests/test_gpu_visibility.py (a library module, no tests of its own): chosen so that in every
case both answers, occluded and open, make up a good share of the rays, under +inf and under the scene's finite distance, which is
short enough to open rays that +inf closes.  The GPU test asserts those shares on the expected bytes before it looks at the product."""
import numpy as np

import prt_amd
import prt_bake_ref as BR
import prt_hostile_shade as HS

F = np.float32
U = np.uint32
N_POINTS = 96
ATRIUM_TRIS = 2000  # the smallest library stand-in with an alpha-tested texture (tests/test_gpu_scene_edit.py uses the same)


def atrium():
    return prt_amd.setup_atrium_standin(64, 64, tris=ATRIUM_TRIS)


SCENES = {"plain": lambda: HS.scene("plain"), "box_rr": lambda: HS.scene("box_rr"), "atrium": atrium}
ATRIUM_BOX = None


def atrium_box():
    global ATRIUM_BOX
    if ATRIUM_BOX is None:
        ATRIUM_BOX = np.array(atrium()[0].bbox(), dtype=np.float64).reshape(2, 3)
    return ATRIUM_BOX


def finite_distance(name):
    """The finite maxDistance of scene `name`, in units of the directions of make_sets (whose lengths are 0.7 .. 1.5)."""
    if name == "plain":
        return 0.3
    if name == "box_rr":
        return 1.0
    lo, hi = atrium_box()
    return float(F(0.09 * np.linalg.norm(hi - lo)))


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def make_points(name, nSets, n=N_POINTS, seed=1):
    """n points of scene `name` on and off its surfaces, unit normals, bias 1e-4, 0 and negative, sets over the whole table, one
    point with set = nSets and one with 0xffffffff."""
    rng = np.random.default_rng(seed)
    N = unit(rng, n)
    if name == "plain":  # 80 % on either side of the tilted patch (mesh 1) and facing it, the others over the stage and ON its floor
        P = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.2, 1.5, n), rng.uniform(-1.5, 3.0, n)], axis=1).astype(F)
        on = np.arange(n) % 5 == 4
        P[on, 1], N[on] = 0.0, (0.0, 1.0, 0.0)
        near = np.arange(n) % 5 < 4
        m = int(near.sum())
        side = np.where(rng.random(m) < 0.5, -1.0, 1.0)
        P[near] = np.stack([rng.uniform(-0.25, 0.25, m), rng.uniform(0.8, 1.1, m), -0.65 + side * rng.uniform(0.05, 0.45, m)], axis=1).astype(F)
        towards = np.stack([np.zeros(m), np.zeros(m), -side], axis=1) + 0.3 * rng.normal(size=(m, 3))
        N[near] = (towards / np.linalg.norm(towards, axis=1, keepdims=True)).astype(F)
    elif name == "box_rr":  # inside the closed box, a few ON its floor, and 40 % outside it, which see past it
        P = rng.uniform(-0.8, 0.8, size=(n, 3)).astype(F)
        on = np.arange(n) % 8 == 0
        P[on, 1], N[on] = -1.0, (0.0, 1.0, 0.0)
        out = np.arange(n) % 5 < 2
        P[out] = (unit(rng, int(out.sum())) * rng.uniform(1.8, 3.0, (int(out.sum()), 1))).astype(F)
    else:  # inside the atrium's box, and 40 % above it
        lo, hi = atrium_box()
        P = rng.uniform(lo, hi, size=(n, 3))
        out = np.arange(n) % 5 < 2
        P[out, 1] = hi[1] + rng.uniform(0.01, 0.2, int(out.sum())) * (hi[1] - lo[1])
        P = P.astype(F)
    bias = np.full(n, 1e-4, F)
    bias[::5], bias[3::7] = 0.0, -0.05
    sets = (np.arange(n) % nSets).astype(U)
    sets[30], sets[33] = nSets, 0xffffffff
    return BR.points(P, N, bias, sets)


def make_sets(nSets, K, Cc, seed=2):
    """Directions of lengths 0.7 .. 1.5 around the upper hemisphere (with a -0.0 and a zero direction), positive weights."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(nSets, K, 3))
    d[..., 2] = np.abs(d[..., 2])
    d = (d / np.linalg.norm(d, axis=2, keepdims=True) * rng.uniform(0.7, 1.5, (nSets, K, 1))).astype(F)  # not normalised: tMax is in units of dir
    d[0, 0, 0] = -0.0
    if K > 2:
        d[nSets - 1, 2] = 0.0
    return BR.Sets(d, rng.uniform(0.05, 1.0, size=(nSets, K, Cc)).astype(F))


# ----------------------------------------------------------------------------- the analytic cases (test 5)
def open_case():
    """Points beyond the bounding sphere of the plain stage (it lies within 5 of the origin), each facing away from it, with 64
    cosine-weighted directions and weights 1/64: nothing is in the way, and 64 additions of 2^-6 do not round."""
    rng = np.random.default_rng(12)
    away = unit(rng, 8)
    d, _ = BR.bake_cosine_set(64, rng)
    return BR.points((away * F(50.0)).astype(F), away, 1e-4), BR.Sets(d[None], np.full((1, 64, 1), 1.0 / 64, F))


def closed_case():
    """Points inside the closed box box_rr, below its ceiling and facing it, with 64 directions in a cone of 30 degrees about the
    normal: every ray ends on the face y = 1.  The cone is there for a reason that is the library's, not the test's: the any-hit walk
    tests a node's box with the reference's strict comparison (the exit distance must EXCEED the entry distance), so a leaf whose box
    has no depth -- the faces x = -1, x = 1 and y = -1 of this box, each alone in its leaf -- is never entered by an occlusion ray,
    and prt_hip_query_any, which this call equals byte for byte (test 1), answers "not occluded" for a ray that ends there.  The
    faces y = 1, z = -1 and z = 1 share leaves that have depth."""
    rng = np.random.default_rng(13)
    n, K = 16, 64
    P = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(0.2, 0.7, n), rng.uniform(-0.3, 0.3, n)], axis=1).astype(F)
    N = np.tile(np.array([(0.0, 1.0, 0.0)], F), (n, 1))
    cos_t, phi = rng.uniform(np.cos(np.pi / 6), 1.0, K), rng.uniform(0, 2 * np.pi, K)
    sin_t = np.sqrt(1 - cos_t * cos_t)
    d = np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), cos_t], axis=1).astype(F)
    return BR.points(P, N, 1e-4), BR.Sets(d[None], rng.uniform(0.1, 1.0, (1, K, 2)).astype(F))
