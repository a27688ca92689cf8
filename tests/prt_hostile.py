"""Hostile geometry and rays for the traversal, BVH build and refit tests (tests/test_hostile_cpu.py, tests/test_gpu_hostile.py).

Scenes (unindexed soups, one diffuse material each, seeded with np.random.default_rng(1000 + seed)):
  grid    three meshes of 7, 60 and 300 triangles whose corners are snapped to multiples of 1/4 (coplanar box faces, boxes of zero
          extent, equal slab entries) and whose zero coordinates are -0.0 with probability 1/2
  twins   120 triangles (0-9 with two equal corners, 10-19 collapsed to a point) added twice, plus triangle 50 alone as a third mesh:
          every hit is a tie between coincident triangles of two or three meshes
  flat    two meshes of 200 triangles, one in the plane y = -0.0, one in the plane z = 0.25: root boxes of zero extent
  scaled  the twins positions times 2**-60 and 2**40 (live oracle only)
Rays: 1024 per scene in eight classes of 128 (ray_classes below); stored with the compiled reference's answers in
tests/golden/hostile_rays.npz by tests/golden/make_golden.py, so that the tests do not depend on numpy's generator."""
import os

import numpy as np

import prt_testlib as T

F = np.float32
SCENES = ("grid", "twins", "flat")
SEEDS = (0, 1, 2, 3)
MAX_T = (1e5, 4.0, 7.3992, 1.0)  # per seed
MESH_TRIS = {"grid": (7, 60, 300), "twins": (120, 120, 1), "flat": (200, 200)}
SCALES = {"tiny": F(2.0) ** -60, "huge": F(2.0) ** 40}
RAYS, CLASSES = 1024, 8
GOLDEN_FILE = os.path.join(T.GOLDEN, "hostile_rays.npz")


def _rng(seed):
    return np.random.default_rng(1000 + seed)


def _soup(rng, n, spread=None):
    """n triangles (n, 3, 3) float64: centres uniform in [-1, 1]^3; corners centre + size * normal, size log-uniform in [0.05, 0.9]
    (or the constant `spread`)."""
    centre = rng.uniform(-1.0, 1.0, (n, 1, 3))
    size = np.exp(rng.uniform(np.log(0.05), np.log(0.9), (n, 1, 1))) if spread is None else spread
    return centre + size * rng.normal(size=(n, 3, 3))


def grid_positions(rng):
    """[(raw, snapped)] per mesh, (3n, 3) float32 each: the unsnapped soup and the same soup on the 1/4 grid with -0.0 zeros."""
    out = []
    for n in MESH_TRIS["grid"]:
        raw = _soup(rng, n)
        snap = (np.round(raw * 4) / 4).astype(F)
        snap[(snap == 0) & (rng.random(snap.shape) < 0.5)] = F(-0.0)
        out.append((raw.astype(F).reshape(-1, 3), snap.reshape(-1, 3)))
    return out


def twins_positions(rng):
    tri = _soup(rng, 120, spread=0.3).astype(F)
    tri[0:10, 2] = tri[0:10, 1]  # two equal corners
    tri[10:20, 1] = tri[10:20, 0]  # a point
    tri[10:20, 2] = tri[10:20, 0]
    a = tri.reshape(-1, 3)
    return [a, a.copy(), tri[50].copy()]


def flat_positions(rng):
    a = rng.uniform(-1.0, 1.0, (600, 3)).astype(F)
    b = rng.uniform(-1.0, 1.0, (600, 3)).astype(F)
    a[:, 1] = F(-0.0)
    b[:, 2] = F(0.25)
    return [a, b]


def ray_classes(rng, verts, seed):
    """(org, dir) float32 (1024, 3): eight classes of 128 rays against the vertices `verts` ((V, 3), V a multiple of 3).
      0 axis-aligned +-e_k, the origin's other two coordinates those of a random vertex    4 along an edge of a random triangle, from outside it
      1 one random component zero, the origin's coordinate on that axis a random vertex's  5 from 1e4 times as far away, towards the scene
      2 origin on a random vertex                                                          6 origin on the 1/4 grid
      3 direction towards a random vertex                                                  7 plain random
    Odd seeds normalise the directions."""
    N, k = RAYS, RAYS // CLASSES
    V = len(verts)
    v64 = verts.astype(np.float64)
    org = rng.uniform(-2.5, 2.5, (N, 3))
    d = rng.normal(size=(N, 3))
    rows = np.arange(k)
    # 0
    ax = rng.integers(0, 3, k)
    d[:k] = np.eye(3)[ax] * rng.choice([-1.0, 1.0], (k, 1))
    v = v64[rng.integers(0, V, k)]
    for off in (1, 2):
        org[rows, (ax + off) % 3] = v[rows, (ax + off) % 3]
    # 1
    ax = rng.integers(0, 3, k)
    d[k + rows, ax] = 0.0
    org[k + rows, ax] = v64[rng.integers(0, V, k), ax]
    # 2, 3
    org[2 * k:3 * k] = v64[rng.integers(0, V, k)]
    d[3 * k:4 * k] = v64[rng.integers(0, V, k)] - org[3 * k:4 * k]
    # 4
    tri = rng.integers(0, V // 3, k)  # corner 0 and corner 1 of ONE triangle: the ray runs along that edge, in the triangle's plane
    a, e0 = v64[tri * 3], v64[tri * 3 + 1]
    org[4 * k:5 * k] = a - 2.0 * (e0 - a)
    d[4 * k:5 * k] = e0 - a
    # 5
    org[5 * k:6 * k] *= 1e4
    d[5 * k:6 * k] = -org[5 * k:6 * k] + rng.normal(size=(k, 3))
    # 6
    org[6 * k:7 * k] = np.round(org[6 * k:7 * k] * 4) / 4
    d[np.all(d == 0, axis=1)] = (0.0, 0.0, 1.0)
    if seed % 2:
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(F)
    d[np.all(d == 0, axis=1)] = (0.0, 0.0, 1.0)
    return org.astype(F), d


def generate(name, seed):
    """(positions per mesh, org, dir, max_t) of scene `name` ("grid", "twins", "flat") for `seed`."""
    rng = _rng(seed)
    if name == "grid":
        meshes = [snapped for _, snapped in grid_positions(rng)]
    elif name == "twins":
        meshes = twins_positions(rng)
    else:
        meshes = flat_positions(rng)
    org, d = ray_classes(rng, np.concatenate(meshes), seed)
    return meshes, org, d, float(MAX_T[seed])


def split_meshes(name, verts):
    """The scene's meshes from all of its vertices in order (the golden file stores them concatenated)."""
    out, first = [], 0
    for n in MESH_TRIS[name]:
        out.append(np.ascontiguousarray(verts[first:first + 3 * n], dtype=F))
        first += 3 * n
    assert first == len(verts)
    return out


_golden = None


def golden(name, seed):
    """dict(meshes, org, dir, max_t, single, packet, occluded_single, occluded_packet) of tests/golden/hostile_rays.npz."""
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN_FILE))
    k = f"{name}{seed}_"
    z = _golden
    return dict(meshes=split_meshes(name, z[k + "verts"]), org=z[k + "org"], dir=z[k + "dir"], max_t=float(z[k + "max_t"]),
                single=z[k + "single"].view(T.HIT_DTYPE).reshape(-1), packet=z[k + "packet"].view(T.HIT_DTYPE).reshape(-1),
                occluded_single=z[k + "occluded_single"], occluded_packet=z[k + "occluded_packet"])


def scaled(which, seed):
    """The twins scene of `seed` with positions, ray origins and maxT times SCALES[which] (a power of two: the directions stay)."""
    g = golden("twins", seed)
    s = SCALES[which]
    return [(m * s).astype(F) for m in g["meshes"]], (g["org"] * s).astype(F), g["dir"], float(F(g["max_t"]) * s)


# ----------------------------------------------------------------------------- scenes for the product and the oracle
def soup_mesh(positions, reflection=0, diffuse=(0.7, 0.6, 0.5)):
    """prt_amd.Mesh of an unindexed soup with one material."""
    import prt_amd
    pos = np.ascontiguousarray(positions, dtype=F).reshape(-1, 3)
    idx = np.arange(len(pos), dtype=np.uint32).reshape(-1, 3)
    mat = np.array([T.make_material(diffuse=diffuse, reflection=reflection)], dtype=T.MATERIAL_DTYPE)
    mesh = prt_amd.Mesh.from_arrays(idx, pos, np.zeros(len(idx), dtype=np.uint32), mat.view(prt_amd.MATERIAL_DTYPE))
    mesh.calculate_bounds()
    return mesh


def product_scene(meshes, light=None, reflective=(), size=64):
    """(prt_amd.Scene, Camera at (0, 0, 3) looking down -z, SceneDesc for the oracle) of soups `meshes`; light = direction of a
    directional light or None; meshes named in `reflective` get reflectionType 1."""
    import prt_amd
    scene = prt_amd.Scene()
    for i, pos in enumerate(meshes):
        scene.add(soup_mesh(pos, reflection=int(i in reflective)))
    if light is not None:
        scene.set_directional_light(light, (3.0, 3.0, 2.5))
    camera = prt_amd.Camera().create((0.0, 0.0, 3.0), (0.0, 0.0, -1.0), size, size)
    return scene, camera, T.scene_desc_from_product(scene, camera, 1.0)


# ----------------------------------------------------------------------------- the word comparison
def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def excepted_words(a, b, what=""):
    """Arrays are equal when their 32-bit words are equal, except that a pair of words may differ when both are zero as floats (+0 /
    -0) or both are NaN (sign and payload).  Asserts that; returns the masks (zero pairs, NaN pairs) over the words of `a`."""
    wa, wb = words(a), words(b)
    assert wa.shape == wb.shape, (what, wa.shape, wb.shape)
    fa, fb = wa.view(F), wb.view(F)
    diff = wa != wb
    zero = diff & (fa == 0) & (fb == 0)
    nan = diff & np.isnan(fa) & np.isnan(fb)
    bad = diff & ~zero & ~nan
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {tuple(int(x[0]) for x in np.nonzero(bad))}"
    return zero, nan


def words_equal(a, b, what=""):
    """excepted_words as a count: the number of excepted pairs."""
    zero, nan = excepted_words(a, b, what)
    return int(zero.sum()) + int(nan.sum())


def rays_on_box_planes(nodes_per_mesh, org, d):
    """Number of rays with a zero direction component whose origin coordinate on that axis equals a lower or upper plane of some
    node: the rays whose slab product is 0 * inf = NaN."""
    on = np.zeros(len(org), dtype=bool)
    for ax in range(3):
        planes = np.unique(np.concatenate([np.concatenate([n["lower"][:, ax], n["upper"][:, ax]]) for n in nodes_per_mesh]))
        on |= (d[:, ax] == 0) & np.isin(org[:, ax], planes)
    return int(on.sum())
