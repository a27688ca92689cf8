"""Hostile texture taps and surface fetches for rows a12 / a14 (Mesh::getSurfaceProperties, Texture::sample / testAlpha,
Material::sampleDiffuse / sampleBump): tests/test_hostile_taps_cpu.py, tests/test_gpu_hostile_taps.py.

Everything is deterministic (np.random.default_rng(SEED)); tests/golden/make_golden.py stores the inputs with the answers of the
COMPILED reference (oracle/_ref/ref_shade, the reference's own texture.cpp / material.cpp / mesh.cpp) in tests/golden/hostile_taps.npz,
so that the tests do not depend on numpy's generator staying what it is.

Maps    sizes SIZES, 4 components ("n4": noise; "b4": alpha in flat 4 x 4 blocks; "f4": one alpha byte everywhere) and 1 component
        ("g1": grey noise; "d1": the z^4 height field of a random normal map, texture.cpp:185-200).  Alpha bytes come from ALPHAS.
Scene   mesh 0 has one material per map (diffuseMap = bumpMap = that map; alpha-tested when the map has 4 components) and two triangles
        per material; meshes 1-3 vary vertex normals / texcoords.  See scene_desc().
taps    per map: every value of axis_values(width) as u and of axis_values(height) as v, crossed with a value of the other axis' set
        (even records) or of LATTICE (odd records); on 4-component maps eight records with a non-finite coordinate, which only the
        packet flavour of the alpha test is asked (the single flavour turns NaN into an INT_MIN index: undefined in the reference).
        Padded to a multiple of 8 per map, so that eight consecutive records fill one packet of one material.
bump    direct sampleBump records on the 1-component maps and two 4-component ones: uv at the wrap and in the last row / column,
        duv01 / duv02 from DUVS (axis steps, a diagonal, zero).
surface per triangle the barycentrics BARY (corners, edges, a sum off 1, -0.0); triangles 0-3 of every mesh are degenerate (two equal
        corners, collinear, a point, cancelling vertex normals) -- the only records whose answers may hold NaN.

What is undefined in the reference is left out, and test_hostile_taps_cpu.py asserts that none of it is emitted: a non-finite uv goes
to the packet alpha test alone; no alpha test on a 1-component map.  sample<Vector3f> on a 1-component map reads two bytes past the
last texel: the upload (prt_upload.hip), the oracle (orc_scene_add_texture) and the harness (ref_harness.cpp loadScene) all put 16
zero bytes behind every map, so those two bytes are 0 everywhere."""
import os

import numpy as np

import prt_testlib as T

F = np.float32
SEED = 20261019
SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (16, 16), (37, 29))  # (width, height)
ALPHAS = (0, 125, 126, 127, 128, 129, 255)
LATTICE = (np.arange(-5, 10) * 0.3125).astype(F)
DUVS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), (0.70710677, 0.70710677), (0.0, 0.0))
BARY = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, 0.5, 0.0), (0.0, 0.25, 0.75), (0.5, 0.0, 0.5), (0.2, 0.5, 0.3),
        (0.3, 0.3, 0.3), (1.0, 1.0, 1.0), (-0.0, 1.0, -0.0), (1.0, -0.0, -0.0), (0.33333334, 0.33333334, 0.33333334))
DEGENERATE_TRIS = 4  # triangles 0..3 of every mesh
GOLDEN_FILE = os.path.join(T.GOLDEN, "hostile_taps.npz")
NONFINITE = ((np.nan, 0.3), (0.3, np.nan), (np.inf, 0.5), (0.5, -np.inf), (np.nan, np.nan), (-np.inf, np.inf), (np.nan, 1e30), (-1e30, np.inf))


# ----------------------------------------------------------------------------- maps
def maps():
    """[(name, texels (h, w, comp) uint8)] in the order of the scene's texture table."""
    rng = np.random.default_rng(SEED)
    out = []
    for w, h in SIZES:
        t = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        t[..., 3] = rng.choice(np.array(ALPHAS, dtype=np.uint8), (h, w))
        out.append((f"n4_{w}x{h}", t))
        out.append((f"g1_{w}x{h}", rng.integers(0, 256, (h, w, 1), dtype=np.uint8)))
    for w, h in ((16, 16), (37, 29)):
        t = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        by, bx = np.arange(h)[:, None] // 4, np.arange(w)[None, :] // 4
        t[..., 3] = np.array(ALPHAS, dtype=np.uint8)[(bx + 3 * by) % len(ALPHAS)]
        out.append((f"b4_{w}x{h}", t))
    for (w, h), a in (((1, 1), 127), ((1, 1), 128), ((2, 2), 127), ((3, 5), 126), ((3, 5), 129)):
        t = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        t[..., 3] = a
        out.append((f"f4_{w}x{h}_{a}", t))
    n = rng.integers(0, 256, (16, 16, 3)).astype(F)  # a normal map's bytes -> its height field
    v = F(2.0) * (n * F(1.0 / 255.0) - F(0.5))
    z = v[..., 2] / np.sqrt((v * v).sum(-1)).astype(F)
    out.append(("d1_16x16", (F(255.0) * np.clip(z * z * z * z, F(0), F(1))).astype(np.uint8)[..., None]))
    return out


def cell_classes(tex):
    """Per bilinear cell (h, w) of a 4-component map: 1 = all four alpha bytes >= 128 (pass), 2 = all <= 126 (fail), 3 = all 127,
    0 = mixed; the cell's partners are x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1) (texture.cpp:41-44)."""
    a = tex[..., 3].astype(np.int32)
    h, w = a.shape
    x1, y1 = np.minimum(np.arange(w) + 1, w - 1), np.minimum(np.arange(h) + 1, h - 1)
    four = np.stack([a, a[:, x1], a[y1, :], a[y1][:, x1]])
    lo, hi = four.min(0), four.max(0)
    return np.where(lo >= 128, 1, np.where(hi <= 126, 2, np.where((lo == 127) & (hi == 127), 3, 0)))


# ----------------------------------------------------------------------------- uv
def axis_values(n):
    """The hostile coordinates of an axis with n texels, float32: every texel centre (k + 0.5) / n and edge k / n for k in [-2n, 2n]
    with both float neighbours; +-0; 1 and its neighbours; +-1e-9 (the fraction rounds to 1.0); +-1e-45; 2^23 + 0.5, 2^22 + 0.5;
    +-2^24; +-1e30."""
    k = np.arange(-2 * n, 2 * n + 1).astype(F)
    base = np.concatenate([(k + F(0.5)) / F(n), k / F(n)]).astype(F)
    near = np.concatenate([base, np.nextafter(base, F(-np.inf)), np.nextafter(base, F(np.inf))])
    one = F(1.0)
    special = np.array([0.0, -0.0, 1.0, np.nextafter(one, F(0)), np.nextafter(one, F(2)), -1.0, 1e-9, -1e-9, 1e-45, -1e-45,
                        2.0 ** 23 + 0.5, 2.0 ** 22 + 0.5, 2.0 ** 24, -2.0 ** 24, 1e30, -1e30], dtype=F)
    return np.concatenate([near, special]).astype(F)


def tap_records(tex_list):
    """(records (N, 4) uint32 {material, u bits, v bits, flags}, first record of every map (len + 1)).  flags 1: uv finite, 2: the map
    has 4 components."""
    recs, first = [], [0]
    for m, (_, t) in enumerate(tex_list):
        h, w, comp = t.shape
        U, V = axis_values(w), axis_values(h)
        uv = []
        for i, u in enumerate(U):
            uv.append((u, V[(7 * i + 3) % len(V)] if i % 2 == 0 else LATTICE[(i // 2) % len(LATTICE)]))
        for i, v in enumerate(V):
            uv.append((U[(5 * i + 1) % len(U)] if i % 2 == 0 else LATTICE[(i // 2 + 7) % len(LATTICE)], v))
        uv = np.array(uv, dtype=F)
        flags = np.full(len(uv), 1 | (2 if comp == 4 else 0), dtype=np.uint32)
        if comp == 4:
            uv = np.concatenate([uv, np.array(NONFINITE, dtype=F)])
            flags = np.concatenate([flags, np.full(len(NONFINITE), 2, dtype=np.uint32)])
        pad = (-len(uv)) % 8
        uv = np.concatenate([uv, np.repeat(uv[:1], pad, axis=0)])
        flags = np.concatenate([flags, np.repeat(flags[:1], pad)])
        r = np.zeros((len(uv), 4), dtype=np.uint32)
        r[:, 0] = m
        r[:, 1:3] = uv.view(np.uint32)
        r[:, 3] = flags
        recs.append(r)
        first.append(first[-1] + len(r))
    return np.concatenate(recs), np.array(first, dtype=np.uint32)


def tap_cells(tex, uv, soa=False):
    """(x0, y0, fraction == 1 on either axis, clamp at 0 on either axis, last column or row) of finite taps at uv (N, 2) on `tex`, in
    float32 as texture.cpp:31-44 computes them."""
    h, w = tex.shape[:2]
    s = (uv[:, 0] - np.floor(uv[:, 0])).astype(F)
    t = (uv[:, 1] - np.floor(uv[:, 1])).astype(F)
    xr, yr = (s * F(w) - F(0.5)).astype(F), (t * F(h) - F(0.5)).astype(F)
    x0, y0 = np.floor(np.maximum(xr, F(0))).astype(np.int64), np.floor(np.maximum(yr, F(0))).astype(np.int64)
    return x0, y0, (s == 1) | (t == 1), (xr < 0) | (yr < 0), (x0 == w - 1) | (y0 == h - 1), (xr == np.floor(xr)) | (yr == np.floor(yr))


def bump_records(tex_list):
    """(N, 16) float32 words {material (as uint32 bits), normal[3], uv[2], duv01[2], duv02[2], dp01[3], dp02[3]}."""
    rng = np.random.default_rng(SEED + 1)
    one = F(1.0)
    rows = []
    for m, (name, t) in enumerate(tex_list):
        if not (name[:2] in ("g1", "d1") or name in ("n4_3x5", "n4_16x16")):
            continue
        h, w = t.shape[:2]
        below = np.nextafter(one, F(0))
        uvs = [(below, 0.5), (0.5, below), (below, below), (0.0, 0.0), ((w - 0.5) / w, (h - 0.5) / h), (-0.0, 1.0), ((w - 1.0) / w, 0.25),
               (0.25, (h - 1.0) / h), (0.5 / w, 0.5 / h), (1e-9, -1e-9), (-0.5 / w, 1.0 + 0.5 / h), (0.37, 0.61)]
        for uv in uvs:
            for k, d01 in enumerate(DUVS):
                d02 = DUVS[(k + 1 + len(rows)) % len(DUVS)]
                v = rng.normal(size=(3, 3))
                v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
                row = np.zeros(16, dtype=F)
                row[0:1] = np.array([m], dtype=np.uint32).view(F)
                row[1:4], row[4:6], row[6:8], row[8:10], row[10:13], row[13:16] = v[0], uv, d01, d02, v[1], v[2]
                rows.append(row)
    return np.array(rows, dtype=F)


# ----------------------------------------------------------------------------- the scene
def materials_for(tex_list):
    rng = np.random.default_rng(SEED + 2)
    mats = []
    for m, (_, t) in enumerate(tex_list):
        kd = (1.0, 1.0, 1.0) if m % 5 == 0 else tuple(rng.uniform(0.0, 1.0, 3))
        mats.append(T.make_material(diffuse=kd, alpha_test=int(t.shape[2] == 4), diffuse_map=m, bump_map=m))
    return np.array(mats, dtype=T.MATERIAL_DTYPE)


def _soup(rng, n, mats_per_tri, sizes, normals, texcoords):
    """An unindexed soup of n triangles: positions, optional unit vertex normals, optional texcoords on the texel edges and centres of
    the triangle's own map (+ a few far and tiny values); triangles 0-3 degenerate, 4-5 with coincident texcoords."""
    pos = rng.uniform(-1.0, 1.0, (n, 3, 3)).astype(F)
    pos[0, 1] = pos[0, 0]                                   # two equal corners: dp01 = normalize(0)
    pos[1, 2] = pos[1, 0] + F(2.0) * (pos[1, 1] - pos[1, 0])  # collinear: a zero cross product
    pos[2, 1] = pos[2, 0]                                   # a point
    pos[2, 2] = pos[2, 0]
    nrm = None
    if normals:
        nrm = rng.normal(size=(n, 3, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(F)
        nrm[3, 1] = -nrm[3, 0]                              # vertex normals that cancel at (0.5, 0.5, 0)
        nrm[3, 2] = 0.0
    tc = None
    if texcoords:
        tc = np.zeros((n, 3, 2), dtype=F)
        for k in range(n):
            w, h = sizes[mats_per_tri[k]]
            ku, kv = rng.integers(-2 * w, 2 * w + 1, 3), rng.integers(-2 * h, 2 * h + 1, 3)
            half = rng.integers(0, 2, (3, 2)) * 0.5
            tc[k, :, 0] = ((ku + half[:, 0]).astype(F) / F(w)).astype(F)
            tc[k, :, 1] = ((kv + half[:, 1]).astype(F) / F(h)).astype(F)
        tc[4, 1] = tc[4, 0]                                 # safeNormalize sees zero
        tc[5, 1] = tc[5, 0]
        tc[5, 2] = tc[5, 0]
        tc[6, 0] = (-0.0, 1.0)
        tc[7, 0] = (1e-9, -1e-9)
        tc[8, 2] = (2.0 ** 24, -2.0 ** 24)
    return pos.reshape(-1, 3), None if nrm is None else nrm.reshape(-1, 3), None if tc is None else tc.reshape(-1, 2)


def scene_desc(tex_list=None, width=32, height=32):
    """T.SceneDesc of the four meshes over the maps: mesh 0 (no normals, texcoords) holds every map's material, two triangles each; mesh 1
    (normals, texcoords), mesh 2 (normals, no texcoords), mesh 3 (neither) hold 20 triangles over three materials (none, grey bump,
    RGBA bump + diffuse)."""
    tex_list = maps() if tex_list is None else tex_list
    rng = np.random.default_rng(SEED + 3)
    sizes_all = [(t.shape[1], t.shape[0]) for _, t in tex_list]
    names = [n for n, _ in tex_list]
    mats0 = materials_for(tex_list)
    meshes = []
    pm = np.arange(2 * len(mats0), dtype=np.uint32) % len(mats0)
    pos, nrm, tc = _soup(rng, len(pm), pm, sizes_all, False, True)
    meshes.append(T.MeshDesc(np.arange(len(pos), dtype=np.uint32), pos, pm, mats0, normals=nrm, texcoords=tc))
    g, c = names.index("g1_3x5"), names.index("n4_16x16")
    small = np.array([T.make_material(diffuse=(0.7, 0.6, 0.5)), T.make_material(diffuse=(0.9, 0.8, 0.7), diffuse_map=g, bump_map=g),
                      T.make_material(diffuse=(0.4, 1.0, 0.3), alpha_test=1, diffuse_map=c, bump_map=c)], dtype=T.MATERIAL_DTYPE)
    sizes_small = [(1, 1), sizes_all[g], sizes_all[c]]
    for normals, texcoords in ((True, True), (True, False), (False, False)):
        pm = np.arange(20, dtype=np.uint32) % 3
        pos, nrm, tc = _soup(rng, 20, pm, sizes_small, normals, texcoords)
        meshes.append(T.MeshDesc(np.arange(len(pos), dtype=np.uint32), pos, pm, small, normals=nrm, texcoords=tc))
    return T.SceneDesc(meshes, cam_pos=(0.0, 0.0, 4.0), cam_dir=(0.0, 0.0, -1.0), width=width, height=height, textures=[t for _, t in tex_list])


def surface_records(desc):
    """(N, 5) uint32 {mesh, prim, i bits, j bits, k bits}: every triangle of meshes 1-3 and every second of mesh 0 with every BARY."""
    rows = []
    b = np.array(BARY, dtype=F).view(np.uint32)
    for m, mesh in enumerate(desc.meshes):
        for p in range(mesh.prim_count):
            if m == 0 and p % 2 and p >= 10:
                continue
            for k in range(len(b)):
                rows.append((m, p, b[k, 0], b[k, 1], b[k, 2]))
    return np.array(rows, dtype=np.uint32)


def degenerate_mask(surface):
    return surface[:, 1] < DEGENERATE_TRIS


def generate():
    """dict of every input array of the fixture."""
    tex_list = maps()
    desc = scene_desc(tex_list)
    taps, first = tap_records(tex_list)
    out = dict(taps=taps, taps_first=first, bump=bump_records(tex_list), surface=surface_records(desc))
    for m, (name, t) in enumerate(tex_list):
        out[f"map{m:02d}_{name}"] = t
    for m, mesh in enumerate(desc.meshes):
        out[f"mesh{m}_positions"] = mesh.positions
        out[f"mesh{m}_prim_material"] = mesh.prim_material
        out[f"mesh{m}_materials"] = mesh.materials.view(np.uint8).reshape(len(mesh.materials), -1)
        if mesh.normals is not None:
            out[f"mesh{m}_normals"] = mesh.normals
        if mesh.texcoords is not None:
            out[f"mesh{m}_texcoords"] = mesh.texcoords
    return out


INPUT_KEYS_EXCLUDED = ("ref_taps", "ref_bump", "ref_surface")


# ----------------------------------------------------------------------------- the fixture
_golden = None


def golden():
    """The fixture as a dict: the inputs of generate() plus ref_taps (N, 12), ref_bump (N, 3), ref_surface (N, 20) uint32 words, the
    compiled reference's answers (ref_shade.cpp names the words)."""
    global _golden
    if _golden is None:
        z = dict(np.load(GOLDEN_FILE))
        z["ref_taps"] = unpack_taps(z.pop("ref_taps_f"), z.pop("ref_taps_a"))
        _golden = z
    return _golden


def pack_taps(words):
    """(N, 12) answer words -> (N, 7) float words [sample3, sample1, sampleDiffuse] and (N,) uint8 alpha bits (1 single, 2 packet)."""
    return np.ascontiguousarray(words[:, [0, 1, 2, 3, 6, 7, 8]]), (words[:, 4] | (words[:, 5] << 1)).astype(np.uint8)


def unpack_taps(f, a):
    w = np.zeros((len(f), 12), dtype=np.uint32)
    w[:, [0, 1, 2, 3, 6, 7, 8]] = f
    w[:, 4], w[:, 5] = a & 1, (a >> 1) & 1
    return w


def golden_maps(z):
    keys = sorted(k for k in z if k.startswith("map"))
    return [(k[6:], z[k]) for k in keys]


def golden_desc(z, width=32, height=32):
    """T.SceneDesc from the fixture's stored arrays (not from the generator)."""
    tex_list = golden_maps(z)
    meshes = []
    for m in range(4):
        pos = z[f"mesh{m}_positions"]
        meshes.append(T.MeshDesc(np.arange(len(pos), dtype=np.uint32), pos, z[f"mesh{m}_prim_material"],
                                 np.ascontiguousarray(z[f"mesh{m}_materials"]).view(T.MATERIAL_DTYPE).reshape(-1),
                                 normals=z.get(f"mesh{m}_normals"), texcoords=z.get(f"mesh{m}_texcoords")))
    return T.SceneDesc(meshes, cam_pos=(0.0, 0.0, 4.0), cam_dir=(0.0, 0.0, -1.0), width=width, height=height, textures=[t for _, t in tex_list])


# ----------------------------------------------------------------------------- the compiled reference (oracle/_ref/ref_shade)
def ref_shade(desc, command, records, out_words):
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        sp, ip, op = (os.path.join(td, x) for x in ("s.prts", "in.bin", "out.bin"))
        desc.write_prts(sp)
        np.ascontiguousarray(records).view(np.uint32).astype("<u4").tofile(ip)
        T.run_ref("ref_shade", command, sp, ip, op)
        return np.fromfile(op, dtype="<u4").reshape(-1, out_words)


# ----------------------------------------------------------------------------- the word comparison
def words_equal_but_nan(a, b, what=""):
    """Tolerance 0: the 32-bit words are equal, except where both are NaN as floats.  Returns the number of NaN pairs."""
    wa, wb = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    assert wa.shape == wb.shape, (what, wa.shape, wb.shape)
    diff = wa != wb
    nan = diff & np.isnan(wa.view(F)) & np.isnan(wb.view(F))
    bad = diff & ~nan
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {tuple(int(x[0]) for x in np.nonzero(bad))}: "
                           f"{wa[bad][:4]} != {wb[bad][:4]}")
    return int(nan.sum())


# ----------------------------------------------------------------------------- upload through the C-ABI descriptor
def upload(tracer, desc, light=None):
    """Upload a T.SceneDesc with its textures through the raw descriptor (prt_amd's host meshes take no maps from arrays); the BVHs come
    from the host builder.  Returns the objects that must stay alive while the descriptor is used."""
    import ctypes as C
    import prt_amd
    L = prt_amd.lib()
    keep, mds = [], (prt_amd.MeshDesc * len(desc.meshes))()
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for i, m in enumerate(desc.meshes):
        nodes_p, cnt, remap_p = C.POINTER(prt_amd.BvhNode)(), C.c_uint32(), C.POINTER(C.c_uint32)()
        assert L.prt_host_bvh_build(m.prim_count, m.indices.ctypes.data_as(C.c_void_p), m.positions.ctypes.data_as(C.c_void_p), 0,
                                    C.byref(nodes_p), C.byref(cnt), C.byref(remap_p)) == 0
        nodes = np.frombuffer(C.string_at(nodes_p, cnt.value * C.sizeof(prt_amd.BvhNode)), dtype=T.NODE_DTYPE).copy()
        remap = np.ctypeslib.as_array(remap_p, shape=(m.prim_count,)).copy()
        L.prt_host_free(nodes_p)
        L.prt_host_free(remap_p)
        md = mds[i]
        md.nodeCount, md.nodes = len(nodes), nodes.ctypes.data_as(C.POINTER(prt_amd.BvhNode))
        md.primCount, md.primRemapping = m.prim_count, remap.ctypes.data_as(C.POINTER(C.c_uint32))
        md.vertexCount, md.indices = m.vertex_count, m.indices.ctypes.data_as(C.POINTER(C.c_uint32))
        md.positions = m.positions.ctypes.data_as(C.POINTER(C.c_float))
        if m.normals is not None:
            md.normals = m.normals.ctypes.data_as(C.POINTER(C.c_float))
        if m.texcoords is not None:
            md.texcoords = m.texcoords.ctypes.data_as(C.POINTER(C.c_float))
        md.materialCount, md.primMaterial = len(m.materials), m.prim_material.ctypes.data_as(C.POINTER(C.c_uint32))
        md.materials = m.materials.ctypes.data_as(C.POINTER(prt_amd.Material))
        keep += [nodes, remap]
        lo, hi = np.minimum(lo, m.positions.min(0)), np.maximum(hi, m.positions.max(0))
    tds = (prt_amd.TextureDesc * max(len(desc.textures), 1))()
    for i, t in enumerate(desc.textures):
        a = np.ascontiguousarray(t, dtype=np.uint8)
        tds[i].width, tds[i].height, tds[i].component = a.shape[1], a.shape[0], a.shape[2]
        tds[i].texels = a.ctypes.data_as(C.POINTER(C.c_uint8))
        keep.append(a)
    sd = prt_amd.SceneDesc()
    sd.meshCount, sd.meshes, sd.textureCount, sd.textures = len(desc.meshes), mds, len(desc.textures), tds
    sd.radius = float(T.OracleScene(desc).radius())  # Scene::getRadius of the same meshes (scene.cpp), from the oracle
    if desc.light is not None:
        sd.hasDirectionalLight = 1
        sd.lightDir[:] = [float(x) for x in desc.light[0]]
        sd.lightIntensity[:] = [float(x) for x in desc.light[1]]
    tracer._chk(tracer._L.prt_hip_upload_scene(tracer._ctx, C.byref(sd)), "prt_hip_upload_scene")
    keep += [mds, tds, sd, desc]
    return keep
