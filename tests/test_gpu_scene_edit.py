"""Scene edits on the MI355X (include/prt_hip.h "scene edits"): prt_hip_update_lights, prt_hip_update_materials and
prt_hip_update_textures must leave the context in exactly the state prt_hip_upload_scene produces from the edited scene.  Everything is
compared at tolerance 0: the device arrays byte for byte against a second ("fresh") context that uploaded the edited Scene, images
and event counts against that context and against the oracle, the environment tables against the compiled reference's
(tests/golden/env_light.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

import prt_amd
import prt_testlib as T
from prt_denoise_ref import DEFAULTS
from prt_env_ref import ENV_SHAPES, env_of
from prt_gpukit import assert_bits_equal, upload
from prt_gpukit import dev, gpu_event_accounting, rows, rows2  # noqa: F401  (fixtures)
from prt_temporal_ref import TDEFAULTS

pytestmark = pytest.mark.gpu
F = np.float32
EINVAL, ESTATE = -2, -5
SHADING = ("mats", "alpha_class", "texels", "env_texels", "env_vertical", "env_horizontal", "env_first_x", "env_first_y", "has_light",
           "has_env", "light_dir", "light_intensity")
EVENTS = ("raysTraced", "occludedTraced", "nBox", "nTri", "nTap")


# (differs from prt_refit_ref.teapot_scene: an environment map on request)
def teapot_scene(size=64, env=None):
    scene, camera, exposure = prt_amd.setup_cornell_box(size, size, teapot_mesh=T.teapot_product_mesh())
    if env is not None:
        scene.set_infinite_area_light(env)
    return scene, camera, exposure


def atrium_scene(size=64, bump=True):
    return prt_amd.setup_atrium_standin(size, size, tris=2000, bump=bump)


def shading_equal(got, want, what):
    for k in SHADING:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), f"{what}: {k} differs"


def geometry_equal(got, want, what):
    for k in ("wnodes", "hot", "tris", "shade", "bump", "root_boxes", "radius"):
        assert got[k].tobytes() == want[k].tobytes(), f"{what}: {k} differs"


def traffic(t):
    img = t.render(8, count_traffic=True)
    return img, {k: t.last_stats[k] for k in EVENTS}


def same_as_fresh_and_oracle(rows, rows2, scene, camera, exposure, what, gbuffers=False):
    """The edited context against a context that uploaded the edited Scene, and against the oracle rendering that Scene."""
    upload(rows2, scene, camera)
    shading_equal(rows.shading_arrays(), rows2.shading_arrays(), what)
    geometry_equal(rows.scene_arrays(), rows2.scene_arrays(), what)
    img, ev = traffic(rows)
    img2, ev2 = traffic(rows2)
    assert_bits_equal(img, img2, f"{what}: counting render against the fresh context")
    assert ev == ev2, (what, ev, ev2)
    o = T.OracleScene(T.scene_desc_from_product(scene, camera, exposure))
    ref, ost = o.render(8)
    assert_bits_equal(img, ref, f"{what}: counting render against the oracle")
    assert {k: ev[k] for k in EVENTS} == {k: ost[k] for k in EVENTS}, (what, ev, ost)
    timed = rows.render(8)
    assert_bits_equal(timed, ref, f"{what}: render against the oracle")
    assert_bits_equal(timed, rows2.render(8), f"{what}: render against the fresh context")
    if gbuffers:
        for kind in (0, 2):
            g = rows.gbuffer(kind)
            assert_bits_equal(g, rows2.gbuffer(kind), f"{what}: gbuffer {kind} against the fresh context")
            assert_bits_equal(g, o.gbuffer(kind, (0, 0, camera.width - 1, camera.height - 1)), f"{what}: gbuffer {kind} against the oracle")
    return timed


# ----------------------------------------------------------------------------- 5. environment replace
def test_environment_replace_equals_a_fresh_upload_and_the_reference(rows, rows2):
    z = np.load(os.path.join(T.GOLDEN, "env_light.npz"))
    sky, black = T.sky_env(64, 32), T.sky_env(48, 24, black_rows=True)
    scene, camera, exposure = teapot_scene(64, sky)
    upload(rows, scene, camera)
    first = rows.render(8)
    scene.set_infinite_area_light(black)  # another size, NaN rows
    rows.update_lights(scene)
    got = rows.shading_arrays()
    assert got["env_vertical"].tobytes() == z["black_rows_vertical"].tobytes()
    assert got["env_horizontal"].tobytes() == z["black_rows_horizontal"].tobytes()
    assert np.isnan(got["env_horizontal"]).any() and got["env_texels"].tobytes() == black.tobytes()
    img = same_as_fresh_and_oracle(rows, rows2, scene, camera, exposure, "black rows")
    assert img.tobytes() != first.tobytes()
    scene.set_infinite_area_light(sky)
    rows.update_lights(scene)
    got = rows.shading_arrays()
    assert got["env_vertical"].tobytes() == z["sky_vertical"].tobytes() and got["env_horizontal"].tobytes() == z["sky_horizontal"].tobytes()
    assert_bits_equal(rows.render(8), first, "back under the sky map")


def test_environment_replace_gives_the_compiled_references_pixels(rows):
    """tests/golden/env_light.npz holds the compiled reference's 16 spp pixels over `rect` of the 96 x 96 Cornell box WITHOUT the
    teapot (the scene of test_gpu_parity's environment test; with the teapot, which is in view, 1100 of the crop's 4096 pixels
    differ from the fixture) under sky_env(64, 32): reached here through an edit from another map."""
    z = np.load(os.path.join(T.GOLDEN, "env_light.npz"))
    scene, camera, _ = prt_amd.setup_cornell_box(96, 96)
    scene.set_infinite_area_light(T.sky_env(48, 24, black_rows=True))
    upload(rows, scene, camera)
    scene.set_infinite_area_light(T.sky_env(64, 32))
    rows.update_lights(scene)
    x0, y0, x1, y1 = (int(v) for v in z["rect"])
    assert (x1 - x0 + 1, y1 - y0 + 1) == (64, 64)
    assert_bits_equal(rows.trace_block(x0, y0, x1, y1, 16), z["rgb"], "crop after the edit against the compiled reference")
    st = rows.last_stats
    assert st["raysTraced"] == int(z["rays"][0]) and st["occludedTraced"] == int(z["rays"][1])


# ----------------------------------------------------------------------------- 6. kernel shapes
@pytest.mark.parametrize("shape", ENV_SHAPES + ["black_row"], ids=str)
def test_environment_tables_of_every_shape_equal_a_fresh_upload(rows, rows2, shape):
    e = env_of(shape)
    scene, camera, _ = prt_amd.setup_cornell_box(48, 48)
    scene.set_infinite_area_light(T.sky_env(8, 4))
    rows.upload_scene(scene)
    scene.set_infinite_area_light(e)
    rows.update_lights(scene)
    rows2.upload_scene(scene)
    got = rows.shading_arrays()
    shading_equal(got, rows2.shading_arrays(), str(shape))
    v, h, fx, fy, flags = prt_amd.env_tables_host(e)
    assert flags == 0 and got["env_first_x"].tolist() == fx.tolist() and int(got["env_first_y"][0]) == fy
    assert got["env_vertical"].tobytes() == v.tobytes() and got["env_horizontal"].tobytes() == h.tobytes()


# ----------------------------------------------------------------------------- 7. refusals
def light_update(scene, mode, w=0, h=0, texels=None):
    u = prt_amd.LightUpdate()
    u.hasDirectionalLight = 1  # a refused call must not apply these either
    u.lightDir[:] = [0.0, 1.0, 0.0]
    u.lightIntensity[:] = [9.0, 9.0, 9.0]
    u.envMode, u.envWidth, u.envHeight = mode, w, h
    u.envTexels = None if texels is None else texels.ctypes.data_as(C.POINTER(C.c_float))
    return u


def test_refused_light_updates_change_nothing(rows):
    sky = T.sky_env(16, 8)
    scene, camera, _ = teapot_scene(48, sky)
    upload(rows, scene, camera)
    before, img = rows.shading_arrays(), rows.render(8)
    rows.accumulate(8)
    inf, nan, black = sky.copy(), sky.copy(), sky.copy()
    inf[3, 5, 0] = np.inf
    nan[3, 5, 1] = np.nan
    black[..., :3] = 0.0
    L = rows._L
    REPLACE = prt_amd.LightUpdate.ENV_REPLACE
    for what, u, word in (("+inf", light_update(scene, REPLACE, 16, 8, inf), "non-decreasing"), ("NaN", light_update(scene, REPLACE, 16, 8, nan), "CDF"),
                          ("black", light_update(scene, REPLACE, 16, 8, black), "non-decreasing"),
                          ("2^28 + 1 texels", light_update(scene, REPLACE, (1 << 28) + 1, 1, None), "too large"),
                          ("NULL texels", light_update(scene, REPLACE, 16, 8, None), "NULL"), ("size 0", light_update(scene, REPLACE, 0, 8, sky), "positive"),
                          ("mode 3", light_update(scene, 3), "envMode")):
        assert L.prt_hip_update_lights(rows._ctx, C.byref(u), None) == EINVAL, what
        assert word in L.prt_hip_last_error().decode(), (what, L.prt_hip_last_error().decode())
    assert L.prt_hip_update_lights(rows._ctx, None, None) == EINVAL
    shading_equal(rows.shading_arrays(), before, "after the refused calls")
    assert (rows.accum_counts() == 8).all()  # a refused call does not even empty the accumulator
    assert_bits_equal(rows.render(8), img, "render after the refused calls")
    fresh = prt_amd.PathTracer()
    try:
        u = light_update(scene, prt_amd.LightUpdate.ENV_KEEP)
        assert fresh._L.prt_hip_update_lights(fresh._ctx, C.byref(u), None) == ESTATE
    finally:
        fresh.close()


# ----------------------------------------------------------------------------- 8. directional light
def test_directional_light_and_environment_on_and_off(rows, rows2):
    scene, camera, exposure = teapot_scene(64)
    scene.set_directional_light(prt_amd._normalize((0.2, 1.0, 0.2)), (16.7, 15.6, 11.7))
    upload(rows, scene, camera)
    images = [rows.render(8)]
    scene.set_directional_light(prt_amd._normalize((-0.4, 0.8, 0.3)), (5.0, 9.0, 14.0))  # direction and intensity
    rows.update_lights(scene)
    images.append(same_as_fresh_and_oracle(rows, rows2, scene, camera, exposure, "another sun"))
    # hasDirectionalLight = 0: emissive light only (the Scene class cannot take a light back: a fresh Scene without one)
    u = prt_amd.LightUpdate()
    u.envMode = prt_amd.LightUpdate.ENV_KEEP
    rows._chk(rows._L.prt_hip_update_lights(rows._ctx, C.byref(u), None), "prt_hip_update_lights")
    dark, _, _ = teapot_scene(64)
    assert not dark.arrays()["has_light"]
    images.append(same_as_fresh_and_oracle(rows, rows2, dark, camera, exposure, "no sun"))
    # an environment light on top, then ENV_NONE with a directional light, then ENV_REPLACE again
    scene.set_infinite_area_light(T.sky_env(64, 32))
    rows.update_lights(scene)
    assert rows.shading_arrays()["has_env"][0] == 1
    images.append(same_as_fresh_and_oracle(rows, rows2, scene, camera, exposure, "sun and sky"))
    scene.set_directional_light(prt_amd._normalize((0.2, 1.0, 0.2)), (16.7, 15.6, 11.7))  # (takes the environment light off the Scene)
    rows.update_lights(scene)
    got = rows.shading_arrays()
    assert got["has_env"][0] == 0 and got["env_texels"].size == 0
    assert_bits_equal(same_as_fresh_and_oracle(rows, rows2, scene, camera, exposure, "ENV_NONE with a sun"), images[0], "the first image again")
    scene.set_infinite_area_light(T.sky_env(48, 24, black_rows=True))
    rows.update_lights(scene)
    images.append(same_as_fresh_and_oracle(rows, rows2, scene, camera, exposure, "ENV_REPLACE again"))
    # env=False leaves the device's environment light alone while the sun changes
    scene.set_directional_light(prt_amd._normalize((0.0, 1.0, 0.5)), (3.0, 3.0, 3.0))
    scene.set_infinite_area_light(T.sky_env(48, 24, black_rows=True))
    before = rows.shading_arrays()
    rows.update_lights(scene, env=False)
    got = rows.shading_arrays()
    for k in ("env_texels", "env_vertical", "env_horizontal", "env_first_x", "env_first_y", "has_env"):
        assert got[k].tobytes() == before[k].tobytes(), k
    assert got["light_dir"].tobytes() != before["light_dir"].tobytes() and got["light_intensity"].tobytes() != before["light_intensity"].tobytes()
    # (under an environment light the path never asks for the directional one, path_tracer.cpp:164-173: this image is the last one's)
    assert_bits_equal(same_as_fresh_and_oracle(rows, rows2, scene, camera, exposure, "ENV_KEEP"), images[-1], "another sun under the same sky")
    same = [(i, j) for i in range(len(images)) for j in range(i) if images[i].tobytes() == images[j].tobytes()]
    assert not same, same  # every other edit is visible


# ----------------------------------------------------------------------------- 9. materials
def edit(scene, mesh, material, **fields):
    m = scene.arrays()["meshes"][mesh]["materials"][material].copy()
    for k, v in fields.items():
        m[k] = v
    scene.set_material(mesh, material, m)


ATRIUM_EDITS = [  # (what, material, fields): the atrium's material 0 is bump-mapped (texture 0), 5.. are alpha-tested (texture 1)
    ("a diffuse colour", 1, dict(diffuse=(0.9, 0.2, 0.1))),
    ("an emissive", 2, dict(emissive=(6.0, 5.0, 4.0))),
    ("diffuse to specular", 3, dict(reflectionType=1)),
    ("specular to diffuse", 3, dict(reflectionType=0)),
    ("another diffuseMap", 4, dict(diffuseMap=1)),
    ("bumpMap on", 1, dict(bumpMap=0)),
    ("bumpMap off", 1, dict(bumpMap=-1)),
    ("the colour of an alpha-tested material", 6, dict(diffuse=(0.2, 0.9, 0.3))),
]


def test_material_edits_on_the_atrium(rows, rows2):
    scene, camera, exposure = atrium_scene()
    mats = scene.arrays()["meshes"][0]["materials"]
    assert mats["bumpMap"][0] == 0 and (mats["alphaTest"][5:] == 1).all() and (mats["diffuseMap"][:5] == -1).all()
    upload(rows, scene, camera)
    last = rows.shading_arrays()["mats"]
    for what, material, fields in ATRIUM_EDITS:
        edit(scene, 0, material, **fields)
        rows.update_materials(scene, [(0, material)])
        same_as_fresh_and_oracle(rows, rows2, scene, camera, exposure, what, gbuffers=True)
        now = rows.shading_arrays()["mats"]
        changed = np.nonzero((now.view(np.uint32) != last.view(np.uint32)).any(axis=1))[0]
        assert changed.tolist() == [material], (what, changed)  # exactly the named record
        last = now
    # several in one call
    edit(scene, 0, 0, diffuse=(0.3, 0.3, 0.8))
    edit(scene, 0, 2, emissive=(0.0, 0.0, 0.0))
    rows.update_materials(scene, [(0, 2), (0, 0)])
    same_as_fresh_and_oracle(rows, rows2, scene, camera, exposure, "two materials in one call", gbuffers=True)


def test_material_edits_on_the_cornell_box(rows, rows2):
    scene, camera, exposure = teapot_scene(48)
    upload(rows, scene, camera)
    last = rows.render(8)  # (every surface of this scene is in view)
    box = scene.arrays()["meshes"][0]["materials"]
    dark = int(np.nonzero(~(box["emissive"] > 0).any(axis=1))[0][0])  # a wall
    for what, mesh, material, fields in (("a wall's colour", 0, dark, dict(diffuse=(0.1, 0.7, 0.7))), ("a glowing wall", 0, dark, dict(emissive=(2.0, 1.0, 0.5))),
                                         ("a diffuse teapot", 1, 0, dict(reflectionType=0)), ("a mirror wall", 0, dark, dict(reflectionType=1))):
        edit(scene, mesh, material, **fields)
        rows.update_materials(scene, [(mesh, material)])
        img = same_as_fresh_and_oracle(rows, rows2, scene, camera, exposure, what, gbuffers=True)
        assert img.tobytes() != last.tobytes(), what
        last = img


def test_refused_material_updates_change_nothing(rows):
    scene, camera, _ = atrium_scene(48, bump=False)  # alpha-masked, one texture, NO bump records
    mats = scene.arrays()["meshes"][0]["materials"]
    assert (mats["bumpMap"] < 0).all() and mats["alphaTest"][5] == 1 and mats["diffuseMap"][5] == 0 and len(scene.arrays()["textures"]) == 1
    upload(rows, scene, camera)
    before, geometry, img = rows.shading_arrays(), rows.scene_arrays(), rows.render(8)
    rows.accumulate(8)
    L = rows._L

    def up(mesh=0, material=1, **fields):
        u = prt_amd.MaterialUpdate()
        u.mesh, u.material = mesh, material
        m = mats[min(material, len(mats) - 1)].copy()
        for k, v in fields.items():
            m[k] = v
        u.value = prt_amd.Material.from_buffer_copy(m.tobytes())
        return u

    bad = [([], "no material"), ([up(mesh=1)], "mesh index"), ([up(material=len(mats))], "material index"), ([up(), up(diffuse=(1, 0, 0))], "twice"),
           ([up(alphaTest=1, diffuseMap=0)], "alphaTest"), ([up(material=5, alphaTest=0)], "alphaTest"), ([up(material=5, diffuseMap=-1)], "diffuseMap"),
           ([up(diffuseMap=1)], "texture index"), ([up(bumpMap=1)], "texture index"), ([up(bumpMap=0)], "bump"), ([up(reflectionType=3)], "reflectionType"),
           ([up(diffuse=(1, 1, 1)), up(material=2, reflectionType=7)], "reflectionType")]  # a bad second update refuses the first one too
    for ups, word in bad:
        arr = (prt_amd.MaterialUpdate * max(len(ups), 1))(*ups)
        assert L.prt_hip_update_materials(rows._ctx, len(ups), arr, None) == EINVAL, word
        assert word in L.prt_hip_last_error().decode(), (word, L.prt_hip_last_error().decode())
    assert L.prt_hip_update_materials(rows._ctx, 1, None, None) == EINVAL
    shading_equal(rows.shading_arrays(), before, "after the refused calls")
    geometry_equal(rows.scene_arrays(), geometry, "after the refused calls")
    assert (rows.accum_counts() == 8).all()
    assert_bits_equal(rows.render(8), img, "render after the refused calls")
    fresh = prt_amd.PathTracer()
    try:
        arr = (prt_amd.MaterialUpdate * 1)(up())
        assert fresh._L.prt_hip_update_materials(fresh._ctx, 1, arr, None) == ESTATE
        tex = prt_amd.TextureUpdate()
        assert fresh._L.prt_hip_update_textures(fresh._ctx, 1, C.byref(tex), None) == ESTATE
    finally:
        fresh.close()
    arr = (prt_amd.MaterialUpdate * 1)(up())  # and the accepted call still works: the uploaded value, the same image
    assert L.prt_hip_update_materials(rows._ctx, 1, arr, None) == 0
    shading_equal(rows.shading_arrays(), before, "an update with the uploaded value")
    assert_bits_equal(rows.render(8), img, "an update with the uploaded value")


# ----------------------------------------------------------------------------- 10. textures
def test_texture_repaint_equals_a_fresh_upload(rows, rows2):
    scene, camera, exposure = atrium_scene()
    a = scene.arrays()
    leaf = a["textures"][1]
    assert leaf.shape[2] == 4 and a["meshes"][0]["materials"]["diffuseMap"][5] == 1
    upload(rows, scene, camera)
    old = rows.shading_arrays()
    rng = np.random.default_rng(12)
    paint = rng.integers(0, 256, leaf.shape, dtype=np.uint8)
    # alpha in blotches, so that cells of every class occur, with the three bytes around the threshold among them
    blot = np.repeat(np.repeat(rng.choice(np.array([0, 126, 127, 128, 255], np.uint8), (leaf.shape[0] // 8, leaf.shape[1] // 8)), 8, 0), 8, 1)
    paint[..., 3] = blot
    paint[::37, ::29, 3] = 127
    for v in (126, 127, 128):
        assert (paint[..., 3] == v).any()
    scene.set_texture_texels(1, paint)
    rows.update_textures(scene, [1])
    got = rows.shading_arrays()
    assert got["alpha_class"].tobytes() != old["alpha_class"].tobytes() and got["texels"].tobytes() != old["texels"].tobytes()
    classes = (got["alpha_class"][:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3
    assert {0, 1, 2} <= set(np.unique(classes).tolist())
    same_as_fresh_and_oracle(rows, rows2, scene, camera, exposure, "a repainted alpha texture", gbuffers=True)
    # the bump texture (one component, no class words) and the alpha texture in one call
    bump = rng.integers(0, 256, a["textures"][0].shape, dtype=np.uint8)
    scene.set_texture_texels(0, bump)
    scene.set_texture_texels(1, leaf)
    rows.update_textures(scene, [0, 1])
    same_as_fresh_and_oracle(rows, rows2, scene, camera, exposure, "both textures in one call", gbuffers=True)
    # refusals
    before = rows.shading_arrays()
    L = rows._L
    bytes_ = np.ascontiguousarray(paint)

    def up(texture=1, w=leaf.shape[1], h=leaf.shape[0], comp=4, texels=bytes_):
        u = prt_amd.TextureUpdate()
        u.texture, u.width, u.height, u.component = texture, w, h, comp
        u.texels = None if texels is None else texels.ctypes.data_as(C.POINTER(C.c_uint8))
        return u

    for ups, word in (([], "no texture"), ([up(texture=2)], "texture index"), ([up(w=leaf.shape[1] // 2)], "differs"), ([up(h=1)], "differs"),
                      ([up(comp=3)], "differs"), ([up(texels=None)], "NULL"), ([up(), up()], "twice"), ([up(texture=0, comp=1), up(texture=0, comp=1)], "twice")):
        arr = (prt_amd.TextureUpdate * max(len(ups), 1))(*ups)
        assert L.prt_hip_update_textures(rows._ctx, len(ups), arr, None) == EINVAL, word
        assert word in L.prt_hip_last_error().decode(), (word, L.prt_hip_last_error().decode())
    shading_equal(rows.shading_arrays(), before, "after the refused texture updates")


# ----------------------------------------------------------------------------- 11. invalidation
def test_what_the_edits_invalidate(rows, rows2):
    scene, camera, exposure = atrium_scene()
    scene.set_infinite_area_light(T.sky_env(16, 8))
    upload(rows, scene, camera)
    leaf = scene.arrays()["textures"][1]
    guides = (np.full((64, 64, 3), 0.5, F), np.full((64, 64, 3), 0.25, F))
    position = np.ones((64, 64, 4), F)

    def sampled_state(seed):
        """An accumulator bound to `seed`, a history AND a pending record, host planes."""
        rows.accum_reset()
        rows.seed = seed
        for k in range(2):
            rows.adaptive_pass(8, 0.0, 8 * (k + 1), 8 * (k + 1), 0.01)
        rows.denoise_temporal(exposure=exposure, **TDEFAULTS, **DEFAULTS)
        rows.history_import(rows.history_export(1))
        rows.set_denoise_guides(*guides)
        rows.set_denoise_position(position)
        assert (rows.accum_counts() == 16).all()
        rows.history_export(0), rows.history_export(1)

    def emptied(seed):
        assert (rows.accum_counts() == 0).all() and rows.accum_export()["seed"] == 0
        for which in (0, 1):
            cam = prt_amd.CameraDesc()
            plane = np.zeros((64, 64, 4), F)
            p = plane.ctypes.data_as(C.c_void_p)
            assert rows._L.prt_hip_history_export(rows._ctx, which, C.byref(cam), p, p, p) == ESTATE, which
        rows.seed = seed
        rows.accumulate(8)  # another seed is accepted
        assert rows.accum_export()["seed"] == seed

    try:
        sampled_state(101)
        scene.set_directional_light(prt_amd._normalize((0.3, 1.0, 0.1)), (4.0, 4.0, 4.0))
        scene.set_infinite_area_light(T.sky_env(16, 8))
        rows.update_lights(scene)
        emptied(202)
        for got, want in zip(rows.denoise_guides(8), guides):  # planes the host set survive a light edit
            assert_bits_equal(got, want, "host guides after update_lights")
        assert_bits_equal(rows.denoise_position(), position, "host position plane after update_lights")
        rows.set_denoise_guides(None, None)
        rows.set_denoise_position(None)

        sampled_state(303)
        edit(scene, 0, 1, diffuse=(0.9, 0.1, 0.1))
        rows.update_materials(scene, [(0, 1)])
        emptied(404)
        upload(rows2, scene, camera)
        rows2.seed = 404
        rows2.accumulate(8)
        for got, want, what in zip(rows.denoise_guides(8), rows2.denoise_guides(8), ("albedo", "normal")):  # the host's planes were dropped
            assert_bits_equal(got, want, f"{what} guide after update_materials")
            assert got.tobytes() != guides[0].tobytes() and got.tobytes() != guides[1].tobytes()
        assert_bits_equal(rows.denoise_position(), rows2.denoise_position(), "position plane after update_materials")

        sampled_state(505)
        scene.set_texture_texels(1, np.ascontiguousarray(leaf[::-1]))
        rows.update_textures(scene, [1])
        emptied(606)
        upload(rows2, scene, camera)
        rows2.seed = 606
        rows2.accumulate(8)
        for got, want, what in zip(rows.denoise_guides(8), rows2.denoise_guides(8), ("albedo", "normal")):
            assert_bits_equal(got, want, f"{what} guide after update_textures")
        assert_bits_equal(rows.denoise_position(), rows2.denoise_position(), "position plane after update_textures")
    finally:
        rows.seed = rows2.seed = 12345


# ----------------------------------------------------------------------------- 12. a caller's stream
def test_render_update_render_on_a_callers_stream(rows, rows2, dev):
    scene, camera, _ = teapot_scene(64, T.sky_env(64, 32))
    upload(rows, scene, camera)
    old = rows.render(8)
    scene.set_infinite_area_light(T.sky_env(48, 24, black_rows=True))
    scene_new = scene
    upload(rows2, scene_new, camera)
    new = rows2.render(8)
    assert old.tobytes() != new.tobytes()
    nbytes = 64 * 64 * 3 * 4
    stream, first, second = dev.stream(), dev.alloc(nbytes), dev.alloc(nbytes)
    rows.render_async(0, 0, 63, 63, 8, d_rgb=first, stream=stream)  # the old scene, queued ahead
    rows.update_lights(scene_new, stream=stream)
    rows.render_async(0, 0, 63, 63, 8, d_rgb=second, stream=stream)
    got = [np.zeros((64, 64, 3), F), np.zeros((64, 64, 3), F)]
    for dst, src in zip(got, (first, second)):
        dev.download_async(dst, src, stream)
    dev.synchronize(stream)
    rows.stats()
    assert_bits_equal(got[0], old, "the render queued before the edit")
    assert_bits_equal(got[1], new, "the render queued after the edit")
