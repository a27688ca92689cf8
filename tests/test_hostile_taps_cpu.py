"""Rows a12 / a14 without a GPU (tests/prt_hostile_taps.py): the generator reproduces the stored inputs and emits nothing the reference
leaves undefined; the oracle's row functions (orc_x_*) equal the COMPILED reference's answers in tests/golden/hostile_taps.npz word for
word; every cell class and uv class occurs; and, where the reference harnesses are built (oracle/_ref), ref_shade reproduces the stored
answers, the host mirror's savePpm / normal-to-bump / alpha flag equal the reference's, and ref_path_real -- the reference's OWN surface
fetch and texture taps in a whole render -- reproduces the committed radiance, G-buffer and scene-digest fixtures byte for byte."""
import ctypes as C
import functools
import hashlib
import os
import struct

import numpy as np
import pytest

import prt_amd
import prt_hostile_taps as H
import prt_testlib as T

F = np.float32
need_ref_shade = pytest.mark.skipif(T.ref_binary("ref_shade") is None, reason="oracle/_ref/ref_shade is not built (no reference sources here)")
need_ref_real = pytest.mark.skipif(T.ref_binary("ref_path_real") is None, reason="oracle/_ref/ref_path_real is not built (no reference sources here)")

# how often every class must occur among the stored records (counted from the fixture)
MIN_CELL_CLASS = {"pass": 400, "fail": 400, "mixed": 1500, "all127": 40}
MIN_UV_CLASS = {"fraction rounds to 1": 100, "clamp at 0": 1500, "last column or row": 1500, "on a texel centre": 1000, "width or height 1": 300,
                "non-finite": 8 * 14, "beyond 2^22": 150}


@pytest.fixture(scope="module", autouse=True)
def built():
    prt_amd.build()


@functools.lru_cache(maxsize=None)
def fixture():
    z = H.golden()
    return z, H.golden_maps(z), H.golden_desc(z)


def padded(t):
    """A map's bytes with the 16 zero bytes every holder of a map puts behind it."""
    return np.concatenate([np.ascontiguousarray(t, dtype=np.uint8).reshape(-1), np.zeros(16, dtype=np.uint8)])


def oracle_lib():
    L = T.oracle()
    vp, f = C.c_void_p, C.c_float
    L.orc_x_tex_sample3.argtypes = [C.c_int32] * 3 + [vp, f, f, vp]
    L.orc_x_tex_sample3.restype = None
    L.orc_x_tex_sample1.argtypes = [C.c_int32] * 3 + [vp, f, f]
    L.orc_x_tex_sample1.restype = f
    L.orc_x_tex_test_alpha.argtypes = [C.c_int32] * 3 + [vp, f, f, C.c_int]
    L.orc_x_tex_test_alpha.restype = C.c_int
    L.orc_x_sample_diffuse.argtypes = [vp] + [C.c_int32] * 3 + [vp, f, f, vp]
    L.orc_x_sample_diffuse.restype = None
    L.orc_x_sample_bump.argtypes = [vp] + [C.c_int32] * 3 + [vp] * 7
    L.orc_x_sample_bump.restype = None
    L.orc_x_get_surface.argtypes = [vp, C.c_uint32, f, f, f, vp, vp, vp, vp, vp, vp, vp]
    L.orc_x_get_surface.restype = None
    return L


# ----------------------------------------------------------------------------- the generator and the fixture
def test_generator_reproduces_the_stored_inputs():
    z, _, _ = fixture()
    g = H.generate()
    stored = {k for k in z if not k.startswith("ref_")}
    assert stored == set(g), stored ^ set(g)
    for k, v in g.items():
        assert v.dtype == z[k].dtype and v.shape == z[k].shape and v.tobytes() == z[k].tobytes(), k
    assert os.path.getsize(H.GOLDEN_FILE) <= os.path.getsize(os.path.join(T.GOLDEN, "hostile_rays.npz"))


def test_generator_emits_nothing_the_reference_leaves_undefined():
    z, tex, desc = fixture()
    taps = z["taps"]
    uv = taps[:, 1:3].view(F)
    finite = np.isfinite(uv).all(axis=1)
    comp = np.array([tex[m][1].shape[2] for m in taps[:, 0]])
    assert ((taps[:, 3] & 1 == 1) == finite).all(), "the single flavours are asked of finite uv only, and of all of them"
    assert ((taps[:, 3] & 2 == 2) == (comp == 4)).all(), "the alpha tests are asked of 4-component maps only, and of all their records"
    assert not (taps[:, 3] & ~np.uint32(3)).any() and (taps[:, 3] != 0).all()
    assert len(taps) % 8 == 0 and (taps[:, 0].reshape(-1, 8) == taps[::8, :1]).all(), "a packet of 8 records names one material"
    assert (z["taps_first"] % 8 == 0).all() and z["taps_first"][-1] == len(taps)
    mats0 = desc.meshes[0].materials
    assert len(mats0) == len(tex) and (mats0["diffuseMap"] == np.arange(len(tex))).all() and (mats0["bumpMap"] == np.arange(len(tex))).all()
    assert (mats0["alphaTest"] == [int(t.shape[2] == 4) for _, t in tex]).all()
    for m in desc.meshes:  # no alpha-tested material names a 1-component map
        for mt in m.materials:
            assert not mt["alphaTest"] or tex[mt["diffuseMap"]][1].shape[2] == 4
    b = z["bump"]
    assert np.isfinite(b[:, 1:]).all() and (b[:, 0].view(np.uint32) < len(tex)).all()
    s = z["surface"]
    assert np.isfinite(s[:, 2:].view(F)).all() and all(s[i, 1] < desc.meshes[s[i, 0]].prim_count for i in range(len(s)))
    assert {(w, h) for _, t in tex for h, w in [t.shape[:2]]} == set(H.SIZES)
    assert {t.shape[2] for _, t in tex} == {1, 4}
    alphas = np.unique(np.concatenate([t[..., 3].reshape(-1) for _, t in tex if t.shape[2] == 4]))
    assert set(alphas) == set(H.ALPHAS)


def test_nan_words_only_in_the_degenerate_surface_class():
    z, _, _ = fixture()
    assert not np.isnan(z["ref_taps"][:, [0, 1, 2, 3, 6, 7, 8]].view(F)).any()
    assert not np.isnan(z["ref_bump"].view(F)).any()
    s = z["ref_surface"].view(F)
    deg = H.degenerate_mask(z["surface"])
    nan_rows = np.isnan(np.delete(s, 5, axis=1)).any(axis=1)
    assert not nan_rows[~deg].any(), "a NaN outside the degenerate triangles"
    assert nan_rows[deg].any(), "the degenerate class shows no NaN at all"
    print("surface records with a NaN word:", int(nan_rows.sum()), "of", int(deg.sum()), "degenerate records")


def test_every_cell_class_and_uv_class_occurs():
    z, tex, _ = fixture()
    taps, ref = z["taps"], z["ref_taps"]
    cells = dict.fromkeys(MIN_CELL_CLASS, 0)
    uvc = dict.fromkeys(MIN_UV_CLASS, 0)
    decided = {1: 0, 2: 0}
    for m, (name, t) in enumerate(tex):
        r = taps[z["taps_first"][m]:z["taps_first"][m + 1]]
        a = ref[z["taps_first"][m]:z["taps_first"][m + 1]]
        fin = (r[:, 3] & 1) == 1
        uv = r[fin, 1:3].view(F)
        x0, y0, one, clamp, last, centre = H.tap_cells(t, uv)
        assert (x0 >= 0).all() and (x0 < t.shape[1]).all() and (y0 >= 0).all() and (y0 < t.shape[0]).all()
        uvc["fraction rounds to 1"] += int(one.sum())
        uvc["clamp at 0"] += int(clamp.sum())
        uvc["last column or row"] += int(last.sum())
        uvc["on a texel centre"] += int(centre.sum())
        uvc["width or height 1"] += len(uv) if 1 in t.shape[:2] else 0
        uvc["non-finite"] += int((~fin).sum())
        uvc["beyond 2^22"] += int((np.abs(uv) >= 2.0 ** 22).any(axis=1).sum())
        if t.shape[2] == 4:
            cls = H.cell_classes(t)[y0, x0]
            for key, c in (("mixed", 0), ("pass", 1), ("fail", 2), ("all127", 3)):
                cells[key] += int((cls == c).sum())
            # the shortcut the device takes is sound: a one-sided cell decides like the reference's blend, in both flavours
            for c, want in ((1, 1), (2, 0)):
                assert (a[fin][cls == c][:, 4:6] == want).all(), (name, c)
                decided[c] += int((cls == c).sum())
            assert (a[fin][cls == 3][:, 4:6] == 0).all(), "a blend of four bytes of 127 never exceeds 127"
    print("cell classes:", cells, "uv classes:", uvc)
    for k, n in MIN_CELL_CLASS.items():
        assert cells[k] >= n, (k, cells[k])
    for k, n in MIN_UV_CLASS.items():
        assert uvc[k] >= n, (k, uvc[k])


# ----------------------------------------------------------------------------- the oracle against the compiled reference's answers
def test_oracle_taps_equal_the_reference_answers():
    z, tex, desc = fixture()
    L = oracle_lib()
    taps = z["taps"]
    uv = taps[:, 1:3].view(F)
    got = np.zeros((len(taps), 12), dtype=np.uint32)
    bufs = [padded(t) for _, t in tex]
    out3 = np.zeros(3, dtype=F)
    for i in range(len(taps)):
        m, flags = int(taps[i, 0]), int(taps[i, 3])
        h, w, comp = tex[m][1].shape
        p, u, v = T.vptr(bufs[m]), float(uv[i, 0]), float(uv[i, 1])
        if flags & 1:
            L.orc_x_tex_sample3(w, h, comp, p, u, v, T.vptr(out3))
            got[i, 0:3] = out3.view(np.uint32)
            got[i, 3] = np.array([L.orc_x_tex_sample1(w, h, comp, p, u, v)], dtype=F).view(np.uint32)[0]
            if flags & 2:
                got[i, 4] = L.orc_x_tex_test_alpha(w, h, comp, p, u, v, 0)
            L.orc_x_sample_diffuse(T.vptr(np.ascontiguousarray(desc.meshes[0].materials[m]["diffuse"])), w, h, comp, p, u, v, T.vptr(out3))
            got[i, 6:9] = out3.view(np.uint32)
        if flags & 2:
            got[i, 5] = L.orc_x_tex_test_alpha(w, h, comp, p, u, v, 1)
    assert H.words_equal_but_nan(got, z["ref_taps"], "oracle taps") == 0


def test_oracle_bump_equals_the_reference_answers():
    z, tex, _ = fixture()
    L = oracle_lib()
    b = z["bump"]
    got = np.zeros((len(b), 3), dtype=F)
    bufs = [padded(t) for _, t in tex]
    for i in range(len(b)):
        m = int(b[i, :1].view(np.uint32)[0])
        h, w, comp = tex[m][1].shape
        r = np.ascontiguousarray(b[i])
        L.orc_x_sample_bump(T.vptr(r[1:4].copy()), w, h, comp, T.vptr(bufs[m]), T.vptr(r[4:6].copy()), T.vptr(r[6:8].copy()), T.vptr(r[8:10].copy()),
                            T.vptr(r[10:13].copy()), T.vptr(r[13:16].copy()), T.vptr(got[i]))
    assert H.words_equal_but_nan(got, z["ref_bump"], "oracle sampleBump") == 0


def test_oracle_surface_equals_the_reference_answers():
    z, tex, desc = fixture()
    L = oracle_lib()
    s = z["surface"]
    bary = s[:, 2:].view(F)
    bufs = [padded(t) for _, t in tex]
    oms = [L.orc_mesh_create(m.prim_count, m.vertex_count, len(m.materials), T.vptr(m.indices), T.vptr(m.positions), T.vptr(m.normals),
                             T.vptr(m.texcoords), T.vptr(m.prim_material), T.vptr(m.materials)) for m in desc.meshes]
    got = np.zeros((len(s), 20), dtype=np.uint32)
    g = got.view(F)
    mat = C.c_uint32()
    for i in range(len(s)):
        mesh = desc.meshes[s[i, 0]]
        row = g[i]
        L.orc_x_get_surface(oms[s[i, 0]], int(s[i, 1]), float(bary[i, 0]), float(bary[i, 1]), float(bary[i, 2]), T.vptr(row[0:3]), C.byref(mat),
                            T.vptr(row[3:5]), T.vptr(row[6:8]), T.vptr(row[8:10]), T.vptr(row[10:13]), T.vptr(row[13:16]))
        got[i, 5] = mat.value
        bm = int(mesh.materials[mat.value]["bumpMap"])
        h, w, comp = tex[bm][1].shape if bm >= 0 else (0, 0, 0)
        L.orc_x_sample_bump(T.vptr(row[0:3]), w, h, comp, T.vptr(bufs[bm]) if bm >= 0 else None, T.vptr(row[3:5]), T.vptr(row[6:8]), T.vptr(row[8:10]),
                            T.vptr(row[10:13]), T.vptr(row[13:16]), T.vptr(row[16:19]))
    for om in oms:
        L.orc_mesh_destroy(om)
    nan = H.words_equal_but_nan(got, z["ref_surface"], "oracle getSurfaceProperties + sampleBump")
    print("NaN / NaN pairs:", nan)
    assert (got[:, 5] == [desc.meshes[m].prim_material[p] for m, p in s[:, :2]]).all()


# ----------------------------------------------------------------------------- the compiled reference itself
@need_ref_shade
def test_ref_shade_reproduces_the_stored_answers():
    z, _, desc = fixture()
    assert H.ref_shade(desc, "taps", z["taps"], 12).tobytes() == z["ref_taps"].tobytes()
    assert H.ref_shade(desc, "bump", z["bump"], 3).tobytes() == z["ref_bump"].tobytes()
    assert H.ref_shade(desc, "surface", z["surface"], 20).tobytes() == z["ref_surface"].tobytes()


@need_ref_shade
def test_float_map_taps_of_the_reference_equal_the_oracle(tmp_path):
    """Texture::loadExr (through the raw-image loader of ref_stubs.cpp) + sample<Vector3f> on float maps: the environment light's tap."""
    L = T.oracle()
    L.orc_x_tex_sample3f.argtypes = [C.c_int32] * 3 + [C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    L.orc_x_tex_sample3f.restype = None
    rng = np.random.default_rng(5)
    for w, h in ((1, 1), (1, 7), (7, 1), (3, 5), (16, 16)):
        env = rng.uniform(0.0, 50.0, (h, w, 4)).astype(F)
        d = T.SceneDesc([], (0, 0, 0), (0, 0, -1), 8, 8, env=env)
        U, V = H.axis_values(w), H.axis_values(h)
        uv = np.array([(u, V[(7 * i + 3) % len(V)]) for i, u in enumerate(U)] + [(U[(5 * i + 1) % len(U)], v) for i, v in enumerate(V)], dtype=F)
        d.write_env(tmp_path / "e.prte")
        uv.tofile(tmp_path / "uv.bin")
        T.run_ref("ref_shade", "tapsf", tmp_path / "e.prte", tmp_path / "uv.bin", tmp_path / "o.bin")
        ref = np.fromfile(tmp_path / "o.bin", dtype="<u4").reshape(-1, 3)
        got = np.zeros((len(uv), 3), dtype=F)
        for i in range(len(uv)):
            L.orc_x_tex_sample3f(w, h, 4, T.vptr(env), float(uv[i, 0]), float(uv[i, 1]), T.vptr(got[i]))
        assert H.words_equal_but_nan(got, ref, f"float map {w}x{h}") == 0


def ppm_test_image():
    """0, 1, values just past both, denormals, large values, and a ramp: (h, w, 3) float32."""
    one = F(1.0)
    special = np.array([0.0, -0.0, 1.0, np.nextafter(one, F(0)), np.nextafter(one, F(2)), np.nextafter(F(0), one), -np.nextafter(F(0), one), 1e-45, 1e-40,
                        -1e-40, 1e-38, 0.5, 2.0, 254.0 / 255.0, 1e4, 1e10, 3e38, -1.0, -1e-9, 1e-9, 0.99999, 1.00001, 0.0031308, 1.0 / 255.0], dtype=F)
    ramp = (np.arange(3 * 24 * 15 - len(special), dtype=F) / F(64.0)) ** F(2.0) / F(40.0)
    return np.concatenate([special, ramp]).astype(F).reshape(15, 24, 3)


@need_ref_shade
@pytest.mark.parametrize("tonemap", [False, True])
def test_save_ppm_bytes_equal_the_compiled_reference(tmp_path, tonemap):
    img = ppm_test_image()
    img.tofile(tmp_path / "in.bin")
    T.run_ref("ref_shade", "ppm", img.shape[1], img.shape[0], int(tonemap), tmp_path / "in.bin", tmp_path / "ref.ppm")
    want = open(tmp_path / "ref.ppm", "rb").read()
    assert want.startswith(b"P6\n24 15\n255\n") and len(want) == 13 + img.size
    prt_amd.save_ppm(str(tmp_path / "host.ppm"), img, tonemap=tonemap)
    assert open(tmp_path / "host.ppm", "rb").read() == want, "the host mirror's savePpm"
    got, _ = prt_amd.display_host(img, prt_amd.DisplayParams.make(format=0, transfer=0, tonemap=tonemap, gain=1.0))
    assert got.tobytes() == want[13:], "prt_hip_test_display_host with gain 1, transfer 0"


def write_pnm(path, a):
    """Binary PGM / PPM / PAM of a (h, w, c) uint8 array."""
    h, w, c = a.shape
    with open(path, "wb") as f:
        if c == 4:
            f.write(b"P7\nWIDTH %d\nHEIGHT %d\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n" % (w, h))
        else:
            f.write(b"P%d\n%d %d\n255\n" % (5 if c == 1 else 6, w, h))
        f.write(np.ascontiguousarray(a, dtype=np.uint8).tobytes())


def write_prti(path, a):
    h, w, c = a.shape
    with open(path, "wb") as f:
        f.write(b"PRTI" + struct.pack("<3i", w, h, c) + np.ascontiguousarray(a, dtype=np.uint8).tobytes())


def host_load(tmp_path, diffuse=None, bump=None):
    """The host loader (Mesh::loadObj -> the .mtl's maps): (alphaTest flag, textures) of a one-triangle OBJ."""
    with open(tmp_path / "t.mtl", "w") as f:
        f.write("newmtl m\nKd 1 1 1\n" + ("map_Kd kd.pnm\n" if diffuse is not None else "") + ("map_bump bump.pnm\n" if bump is not None else ""))
    with open(tmp_path / "t.obj", "w") as f:
        f.write("mtllib t.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl m\nf 1/1 2/2 3/3\n")
    if diffuse is not None:
        write_pnm(tmp_path / "kd.pnm", diffuse)
    if bump is not None:
        write_pnm(tmp_path / "bump.pnm", bump)
    scene = prt_amd.Scene()
    scene.add(prt_amd.Mesh.load_obj(str(tmp_path / "t.obj")))
    a = scene.arrays()
    return int(a["meshes"][0]["materials"]["alphaTest"][0]), a["textures"]


def ref_load(tmp_path, a, bump):
    write_prti(tmp_path / "in.prti", a)
    T.run_ref("ref_shade", "load", tmp_path / "in.prti", int(bump), tmp_path / "load.bin")
    raw = open(tmp_path / "load.bin", "rb").read()
    w, h, comp, flag = struct.unpack_from("<4i", raw, 0)
    return flag, np.frombuffer(raw, dtype=np.uint8, offset=16).reshape(h, w, comp)


@need_ref_shade
def test_normal_to_bump_of_the_host_loader_equals_the_reference_on_all_rgb_triples(tmp_path):
    """convertNormalToBump (texture.cpp:185-200) on all 2^24 RGB triples, run by the harness; the host loader converts the same image."""
    T.run_ref("ref_shade", "bump24", tmp_path / "b24.bin")
    want = np.fromfile(tmp_path / "b24.bin", dtype=np.uint8)
    i = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=1).astype(np.uint8).reshape(4096, 4096, 3)
    _, textures = host_load(tmp_path, bump=rgb)
    assert len(textures) == 1 and textures[0].shape == (4096, 4096, 1)
    got = textures[0].reshape(-1)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} of 2^24 triples differ, first rgb = {tuple(int(x) for x in rgb.reshape(-1, 3)[bad[0]])}: {got[bad[0]]} != {want[bad[0]]}"
    # and through Texture::load itself on a small RGB map
    small = np.random.default_rng(3).integers(0, 256, (5, 3, 3), dtype=np.uint8)
    _, ref_tex = ref_load(tmp_path, small, True)
    assert ref_tex.shape == (5, 3, 1) and host_load(tmp_path, bump=small)[1][0].tobytes() == ref_tex.tobytes()


@need_ref_shade
@pytest.mark.parametrize("case", ["opaque", "one texel 254", "last texel 0", "rgb"])
def test_alpha_flag_of_the_host_loader_equals_is_alpha_test_required(tmp_path, case):
    a = np.random.default_rng(4).integers(0, 256, (5, 3, 4), dtype=np.uint8)
    a[..., 3] = 255
    if case == "one texel 254":
        a[2, 1, 3] = 254
    elif case == "last texel 0":
        a[4, 2, 3] = 0
    elif case == "rgb":
        a = a[..., :3]
    want_flag, want_tex = ref_load(tmp_path, a, False)
    flag, textures = host_load(tmp_path, diffuse=a)
    assert flag == want_flag == int(case in ("one texel 254", "last texel 0"))
    assert textures[0].tobytes() == want_tex.tobytes() and want_tex.shape[2] == 4


# ----------------------------------------------------------------------------- whole renders by the reference alone
def sha(rgb):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(rgb, dtype="<f4").tobytes()).digest(), dtype=np.uint8)


@need_ref_real
def test_ref_path_real_reproduces_the_radiance_and_gbuffer_fixtures():
    z = np.load(os.path.join(T.GOLDEN, "radiance_c1_crop.npz"))
    rgb, _ = T.ref_render(T.cornell_scene(512, 512, with_teapot=True), 16, tuple(int(v) for v in z["rect"]), seed=12345, stats=False, binary="ref_path_real")
    assert rgb.tobytes() == z["rgb"].tobytes(), "C1 crop"
    g = np.load(os.path.join(T.GOLDEN, "gbuffer.npz"))
    desc = T.cornell_scene(96, 96, with_teapot=True)
    for k in (0, 1, 2):
        assert T.ref_gbuffer(desc, k, tuple(int(v) for v in g["rect"]), binary="ref_path_real").tobytes() == g[f"kind{k}"].tobytes(), f"G-buffer kind {k}"


@need_ref_real
@pytest.mark.parametrize("name,setup,kw,w,h", [("c2", "setup_bunny_standin", dict(tris=20000), 192, 192),
                                              ("c3", "setup_atrium_standin", dict(tris=40000), 192, 108)])
def test_ref_path_real_reproduces_the_scene_digests(name, setup, kw, w, h):
    """The C3-class scene has alpha masks, a bump map and vertex normals: with the reference's own getSurfaceProperties / sampleDiffuse /
    sampleBump / testAlpha serving the whole render, the committed digest (made with those members forwarded to the oracle) must stand."""
    z = np.load(os.path.join(T.GOLDEN, "scene_digests.npz"))
    scene, camera, exposure = getattr(prt_amd, setup)(w, h, **kw)
    desc = T.scene_desc_from_product(scene, camera, exposure)
    rgb, _ = T.ref_render(desc, 16, (0, 0, w - 1, h - 1), seed=12345, stats=False, binary="ref_path_real")
    assert np.array_equal(rgb.astype(np.float64).sum(axis=(1, 2)), z[f"{name}_row_sums"]), "row sums"
    assert (sha(rgb) == z[f"{name}_sha256"]).all(), "sha256 of the float image"
