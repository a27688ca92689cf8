"""The one staging arena of the host-array entry points on the MI355X (prt_amd/csrc/prt_stage.h; the CPU half is
tests/test_stage_cpu.py): calls of every family and of many sizes share one context, and each answers bit for bit what it answers alone
on a fresh context.  A stale slice, a wrong offset or a missing synchronise before a regrow of the arena would show as a difference.
Cornell box with the teapot (two meshes); everything at tolerance 0, compared as bytes."""
import ctypes as C

import numpy as np
import pytest

import prt_amd
import prt_testlib as T
from prt_gpukit import SENTINEL
from prt_gpukit import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
CAM_W, CAM_H = 64, 48
AW = AH = 4  # the atlas


@pytest.fixture(scope="module")
def fresh():
    """fresh() -> a new context with the scene uploaded; all are closed at the end."""
    prt_amd.build()
    scene, camera, _ = prt_amd.setup_cornell_box(CAM_W, CAM_H, teapot_mesh=T.teapot_product_mesh())
    made = []

    def make():
        t = prt_amd.PathTracer(max_depth=6, seed=77)
        t.upload_scene(scene)
        made.append(t)
        return t
    make.camera = camera
    yield make
    for t in made:
        t.close()


def rays(fresh, n):
    return prt_amd.pixel_centre_rays(fresh.camera.desc, (7 * np.arange(n) + 3) % CAM_W, (5 * np.arange(n) // CAM_W + 11) % CAM_H)


# two meshes with 1 and 3 triangles in a 4 x 4 atlas: mesh 0 covers the lower left, mesh 1 the rest in three pieces
UVS = {0: np.array([[(0, 0), (0.6, 0), (0, 0.6)]], F),
       1: np.array([[(1, 1), (0.3, 1), (1, 0.3)], [(0.5, 0.5), (1, 0.1), (1, 0.5)], [(0.1, 0.9), (0.4, 0.6), (0.4, 0.95)]], F)}


def bake_inputs():
    rng = np.random.default_rng(28)
    points = np.array([(0.0, 1.0, 0.0), (0.5, 0.5, 0.2), (-0.6, 1.2, -0.3), (0.2, 1.9, 0.1), (0.0, 0.1, 0.4)], F)
    normals = np.array([(0, 1, 0), (0, 0, 1), (1, 0, 0), (0, -1, 0), (0, 0, 0)], F)
    dirs = rng.normal(size=(3, 3)).astype(F)
    dirs[:, 2] = np.abs(dirs[:, 2]) + F(0.1)
    weights = rng.uniform(0.1, 1.0, size=(3, 2)).astype(F)
    return points, normals, dirs, weights


def values_for(n):
    return np.random.default_rng(6).uniform(-1, 1, size=(n, 3)).astype(F)


# Every step returns its answer as one bytes object.  Steps 5 and 6 hand the rasteriser's output on through `carry`.
def step_any3(t, fresh, carry):
    r = rays(fresh, 3)
    return t.query_any(r["org"], r["dir"], r["tMax"]).tobytes()


def step_nearest1(t, fresh, carry):
    r = rays(fresh, 1)
    hits, surf = t.query_nearest(r["org"], r["dir"], r["tMax"], surface=True)
    return hits.tobytes() + surf.tobytes()


def step_radiance(t, fresh, carry):
    r = rays(fresh, 8)
    return t.query_radiance(r["org"], r["dir"], 8, seed=5).tobytes()


def step_bake(t, fresh, carry):
    points, normals, dirs, weights = bake_inputs()
    out = t.bake(points, normals, dirs, weights, 8, seed=9)
    assert out.shape == (5, 2, 3)
    return out.tobytes()


def step_rasterize(t, fresh, carry):
    texels, hits, counts = t.atlas_rasterize(UVS, AW, AH)
    assert 0 < counts["n"] < AW * AH and set(hits["meshId"]) == {0, 1}
    carry["texels"], carry["hits"] = texels, hits
    return texels.tobytes() + hits.tobytes() + repr(sorted(counts.items())).encode()


def step_points_resolve(t, fresh, carry):
    if "texels" not in carry:  # alone on a fresh context: the rasteriser's output from a context of its own
        step_rasterize(fresh(), fresh, carry)
    pts = t.atlas_points(carry["texels"], carry["hits"], AW, set_tile=2)
    image, mask = t.atlas_resolve(carry["texels"], values_for(len(carry["texels"])), AW, AH, gutter=2)
    return pts.tobytes() + image.tobytes() + mask.tobytes()


def step_nearest4096(t, fresh, carry):
    r = rays(fresh, 4096)
    hits, surf = t.query_nearest(r["org"], r["dir"], r["tMax"], surface=True)
    assert (hits["t"] != -1).any()
    return hits.tobytes() + surf.tobytes()


STEPS = [step_any3, step_nearest1, step_radiance, step_bake, step_rasterize, step_points_resolve, step_nearest4096, step_any3]


def test_one_arena_serves_every_family_and_size(fresh):
    shared, carry = fresh(), {}
    got = [step(shared, fresh, carry) for step in STEPS]  # (the 4096-ray query regrows the arena with work behind it)
    assert got[0] == got[7], "the same three rays answer differently after the arena has served other calls"
    alone = {}
    for k, step in enumerate(STEPS):
        if step not in alone:
            alone[step] = step(fresh(), fresh, {})
        assert got[k] == alone[step], f"step {k + 1} ({step.__name__}) differs from the same call on a fresh context"


def test_a_rasterise_that_owns_no_texel_leaves_the_arrays_alone(fresh):
    t = fresh()
    t.atlas_rasterize(UVS, AW, AH)  # the arena holds texels and hits of an earlier call
    uv = np.array([[(0.2, 0.2), (0.5, 0.5), (0.8, 0.8)]], F)  # A == 0
    rec = (prt_amd.AtlasMesh * 1)(prt_amd.AtlasMesh(meshId=0, primCount=1, uv=uv.ctypes.data))
    texels, hits, counts = np.full(AW * AH, SENTINEL, U), np.full(AW * AH * 6, SENTINEL, U), prt_amd.AtlasCounts()
    rc = t._L.prt_hip_atlas_rasterize(t._ctx, AW, AH, 1, rec, texels.ctypes.data, hits.ctypes.data, C.byref(counts), prt_amd.QUERY_HOST, None)
    assert rc == 0, t._L.prt_hip_last_error()
    assert (counts.n, counts.degenerate, counts.rejected, counts.pairs) == (0, 1, 0, 0)
    assert (texels == SENTINEL).all() and (hits == SENTINEL).all(), "n = 0, and an entry of the caller's arrays was written"


def test_device_array_calls_leave_the_arena_alone(fresh, dev):
    t = fresh()
    want = step_nearest1(fresh(), fresh, {})
    assert step_nearest1(t, fresh, {}) == want  # the arena holds one ray's worth
    points, normals, dirs, weights = bake_inputs()
    pts = prt_amd.make_bake_points(points, normals)
    d, w, table = prt_amd.make_bake_sets(dirs, weights)
    table.dirs, table.weights = dev.upload(d), dev.upload(w)
    out = np.zeros((5, 2, 3), F)
    d_out = dev.upload(out)
    t.bake_async(5, dev.upload(pts), table, d_out, 8, seed=9)
    texels = np.array([0, 5, 10, 15], U)
    image = np.zeros((AH, AW, 3), F)
    d_image = dev.upload(image)
    t.atlas_resolve_async(AW, AH, 4, dev.upload(texels), dev.upload(values_for(4)), 3, 2, d_image, None)  # mask = NULL: the context's scratch mask
    t.stats()  # synchronises the context's stream
    dev.download(out, d_out)
    dev.download(image, d_image)
    assert out.tobytes() == step_bake(fresh(), fresh, {}), "device and host arrays give different sums"
    assert image.tobytes() == fresh().atlas_resolve(texels, values_for(4), AW, AH, gutter=2)[0].tobytes()
    assert step_nearest1(t, fresh, {}) == want, "a host-array query after device-array calls differs from a fresh context's"
