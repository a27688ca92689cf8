"""Scene edits without a GPU (include/prt_hip.h "scene edits"): the entry points and their bindings, the arithmetic the environment
kernels run (prt_amd/csrc/prt_envcdf.h, on the host through prt_hip_test_env_tables_host) against the compiled reference's tables and
against the host mirror's, and the host mirror's Scene.set_material / Scene.set_texture_texels.  Everything at tolerance 0."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import prt_amd
import prt_testlib as T
from prt_env_ref import ENV_SHAPES, env_of

F = np.float32
BAD_VERTICAL, PARTLY_NAN, BAD_ROW = 1, 2, 4


def first_step(cdf):
    """firstStep of prt_hip_upload_scene (light.cpp:96-98, 112-114): the first i >= 1 with !(cdf[i] - cdf[i - 1] == 0), else n."""
    with np.errstate(invalid="ignore"):
        d = cdf[1:] - cdf[:-1]
    hit = np.nonzero(~(d == 0))[0]
    return int(hit[0]) + 1 if len(hit) else len(cdf)


@pytest.fixture(scope="module")
def L():
    prt_amd.build()
    return prt_amd.lib()


def header(name="prt_hip.h"):
    return open(os.path.join(T.ROOT, "include", name)).read()


def struct_fields(hdr, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(",")
        out.append(re.search(r"(\w+)(?:\[\d+\])?$", first.strip()).group(1))
        out += [re.search(r"(\w+)", r).group(1) for r in rest]
    return out


# ----------------------------------------------------------------------------- 1. exports and bindings
def test_entry_points_are_exported_declared_and_bound(L):
    hdr = header()
    for name, sig in (("prt_hip_update_lights", r"\(prt_hip_ctx\* ctx, const prt_light_update\* update, void\* stream\);"),
                      ("prt_hip_update_materials", r"\(prt_hip_ctx\* ctx, uint32_t count, const prt_material_update\* updates, void\* stream\);"),
                      ("prt_hip_update_textures", r"\(prt_hip_ctx\* ctx, uint32_t count, const prt_texture_update\* updates, void\* stream\);")):
        assert name in prt_amd.EXPORTS
        assert re.search(r"int " + name + sig, hdr), name
    assert hdr.index("---- scene edits") > hdr.index("---- geometry updates")  # the new section is the last one
    assert hdr.rindex("prt_hip_update_textures") > hdr.rindex("prt_hip_update_meshes(")
    for struct, binding in (("prt_light_update", prt_amd.LightUpdate), ("prt_material_update", prt_amd.MaterialUpdate),
                            ("prt_texture_update", prt_amd.TextureUpdate)):
        assert struct_fields(hdr, struct) == [n for n, _ in binding._fields_], (struct, struct_fields(hdr, struct))
    for k, mode in enumerate(("KEEP", "NONE", "REPLACE")):
        assert re.search(r"#define PRT_HIP_ENV_%s %d\b" % (mode, k), hdr) and getattr(prt_amd.LightUpdate, "ENV_" + mode) == k
    assert C.sizeof(prt_amd.MaterialUpdate) == 8 + C.sizeof(prt_amd.Material)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", prt_amd.LIB_PATH]).decode()
    for name in ("prt_hip_update_lights", "prt_hip_update_materials", "prt_hip_update_textures", "prt_host_scene_set_material",
                 "prt_host_scene_set_texture_texels"):
        assert f" T {name}\n" in syms, name
    assert "prt_hip_test" not in syms
    test_hdr = header("prt_hip_test.h")
    TL = prt_amd.test_lib()
    for name in ("prt_hip_test_shading_arrays", "prt_hip_test_env_tables_host", "prt_hip_test_edit_profile"):
        assert name in prt_amd.TEST_EXPORTS and name in test_hdr and hasattr(TL, name) and not hasattr(L, name), name
    from prt_amd import _build as B
    assert "prt_edit.hip" in B.SOURCES and "prt_envcdf.h" in B.KERNEL_HEADERS
    # reachable without a device: no context
    light, mat, tex = prt_amd.LightUpdate(), prt_amd.MaterialUpdate(), prt_amd.TextureUpdate()
    assert L.prt_hip_update_lights(None, C.byref(light), None) == -2  # PRT_HIP_EINVAL
    assert L.prt_hip_last_error()
    assert L.prt_hip_update_materials(None, 1, C.byref(mat), None) == -2
    assert L.prt_hip_update_textures(None, 1, C.byref(tex), None) == -2


def test_header_states_the_contract():
    hdr = header()
    block = hdr[hdr.index("---- scene edits"):]
    block = " ".join(block[:block.index("---- */")].replace("\n *", " ").split())
    assert ("after the call the context is in exactly the state prt_hip_upload_scene produces from the uploaded descriptor with these "
            "fields replaced; every device array is the same byte for byte") in block
    for mode in ("PRT_HIP_ENV_KEEP", "PRT_HIP_ENV_NONE", "PRT_HIP_ENV_REPLACE"):
        assert mode in block
    assert "SEQUENTIAL along a row and along the column" in block and "neither a tree reduction nor a parallel scan" in block
    assert "l = sqrtf((r*r + g*g) + b*b)" in block and "no FMA" in block
    assert "A refused call changes nothing" in block and "PRT_HIP_ESTATE without a scene" in block
    inv = block[block.index("What the calls invalidate"):]
    for phrase in ("empty the accumulator and the moments and unbind the estimator", "drop the temporal history AND the pending record",
                   "exports the history before the edit", "prt_hip_update_lights leaves the denoise guides, the position plane",
                   "planes a host had set are dropped", "renders the edited scene"):
        assert phrase in inv, phrase
    reset = hdr[hdr.index("Empties the accumulator"):hdr.index("int prt_hip_accum_reset")]
    for name in ("prt_hip_update_lights", "prt_hip_update_materials", "prt_hip_update_textures"):
        assert name in reset


# ----------------------------------------------------------------------------- 2. against the compiled reference's tables
@pytest.mark.parametrize("name,env", [("sky", lambda: T.sky_env(64, 32)), ("black_rows", lambda: T.sky_env(48, 24, black_rows=True))])
def test_host_tables_equal_the_compiled_reference(L, name, env):
    z = np.load(os.path.join(T.GOLDEN, "env_light.npz"))
    e = env()
    assert tuple(z[name + "_size"][:2]) == (e.shape[1], e.shape[0])
    v, h, fx, fy, flags = prt_amd.env_tables_host(e)
    assert v.tobytes() == z[name + "_vertical"].tobytes()
    assert h.tobytes() == z[name + "_horizontal"].tobytes()
    assert flags == 0
    if name == "black_rows":
        rows = h.reshape(e.shape[0], e.shape[1])
        nan_rows = np.isnan(rows).all(axis=1)
        assert nan_rows.sum() == 13 and not np.isnan(rows[~nan_rows]).any()  # row 1 and the lower half


# ----------------------------------------------------------------------------- 3. against the host mirror
@pytest.mark.parametrize("shape", ENV_SHAPES + ["black_row"], ids=str)
def test_host_tables_equal_the_host_mirror(L, shape):
    e = env_of(shape)
    scene = prt_amd.Scene()
    scene.set_infinite_area_light(e)
    a = scene.arrays()
    v, h, fx, fy, flags = prt_amd.env_tables_host(e)
    assert v.tobytes() == a["env_vertical"].tobytes() and h.tobytes() == a["env_horizontal"].tobytes()
    rows = a["env_horizontal"].reshape(e.shape[0], e.shape[1])
    assert fx.tolist() == [first_step(r) for r in rows]
    assert fy == first_step(a["env_vertical"])
    assert flags == 0
    if shape == "black_row":
        assert np.isnan(rows[5]).all() and fx[5] == 1


def test_host_flags_are_the_uploads_refusals(L):
    e = T.sky_env(16, 8)
    inf, nan, black, neg = e.copy(), e.copy(), e.copy(), e.copy()
    inf[3, 5, 0] = np.inf
    nan[3, 5, 1] = np.nan
    black[..., :3] = 0.0
    flags = lambda m: prt_amd.env_tables_host(m)[4]  # noqa: E731
    assert flags(e) == 0
    # +inf: hsum = inf, invH = 0, 0 * inf = NaN from the texel on -> the row starts with numbers and turns NaN; vert[3] = inf -> NaN
    assert flags(inf) & BAD_ROW and flags(inf) & BAD_VERTICAL
    assert flags(nan) != 0 and flags(black) & BAD_VERTICAL
    # a row that is NaN from its first entry but not throughout cannot come from this arithmetic with finite sums; the rule is
    # exercised where it can be: a NaN in the row's FIRST texel makes hsum NaN and the whole row NaN -- accepted as a row, refused
    # by the vertical table
    first = e.copy()
    first[3, 0, 0] = np.nan
    assert flags(first) == BAD_VERTICAL
    # 1 x 1 black: the vertical table has nothing to compare -- accepted, as the upload accepts the host mirror's tables
    one = np.zeros((1, 1, 4), F)
    assert flags(one) == 0
    with pytest.raises(prt_amd.PrtError):
        prt_amd.env_tables_host(np.zeros((0, 4, 4), F))


# ----------------------------------------------------------------------------- 4. host mirror
def desc_snapshot(scene):
    a = scene.arrays()
    return a, [m["materials"].copy() for m in a["meshes"]], [t.copy() for t in a["textures"]]


def test_scene_set_material_changes_exactly_the_named_entry(L):
    scene, _, _ = prt_amd.setup_atrium_standin(64, 64, tris=2000)
    a, mats, texs = desc_snapshot(scene)
    assert len(texs) == 2 and mats[0]["bumpMap"][0] == 0 and (mats[0]["alphaTest"][5:] == 1).all()
    new = mats[0][4].copy()
    new["diffuse"] = (0.1, 0.2, 0.3)
    new["emissive"] = (4.0, 3.0, 2.0)
    new["reflectionType"] = 1
    new["diffuseMap"] = 1
    new["bumpMap"] = 0
    scene.set_material(0, 4, new)
    b, mats2, texs2 = desc_snapshot(scene)
    assert mats2[0][4].tobytes() == new.tobytes()
    keep = np.arange(len(mats[0])) != 4
    assert mats2[0][keep].tobytes() == mats[0][keep].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(texs, texs2)) and len(texs2) == 2
    for k in ("nodes", "positions", "prim_material", "indices"):
        assert b["meshes"][0][k].tobytes() == a["meshes"][0][k].tobytes()
    back = prt_amd.Material.from_buffer_copy(mats[0][4].tobytes())  # a Material works as well as a numpy record
    scene.set_material(0, 4, back)
    assert desc_snapshot(scene)[1][0].tobytes() == mats[0].tobytes()
    for mesh, material, value in ((1, 0, new), (0, len(mats[0]), new)):
        with pytest.raises(prt_amd.PrtError):
            scene.set_material(mesh, material, value)
    bad = new.copy()
    bad["diffuseMap"] = 2
    with pytest.raises(prt_amd.PrtError):
        scene.set_material(0, 4, bad)
    assert desc_snapshot(scene)[1][0].tobytes() == mats[0].tobytes()


def test_scene_set_texture_texels_changes_exactly_the_named_texture(L):
    scene, _, _ = prt_amd.setup_atrium_standin(64, 64, tris=2000)
    a, mats, texs = desc_snapshot(scene)
    paint = np.random.default_rng(3).integers(0, 256, texs[1].shape, dtype=np.uint8)
    scene.set_texture_texels(1, paint)
    b, mats2, texs2 = desc_snapshot(scene)
    assert texs2[1].tobytes() == paint.tobytes() and texs2[0].tobytes() == texs[0].tobytes()
    assert mats2[0].tobytes() == mats[0].tobytes()
    with pytest.raises(prt_amd.PrtError):
        scene.set_texture_texels(2, paint)
    with pytest.raises(prt_amd.PrtError):
        scene.set_texture_texels(1, paint[:-1])
    assert desc_snapshot(scene)[2][1].tobytes() == paint.tobytes()
