"""Hostile materials and lights for the bounce loop (shade_round in prt_amd/csrc/prt_frame.h; path_tracer.cpp:131-307): the scenes of
tests/test_hostile_shade_cpu.py and tests/test_gpu_hostile_shade.py.  Nothing here draws a random number.

Scenes
  stage  32 x 32, camera at (0, 1.3, 3.2) looking along (0, -0.3, -1).  Mesh 0 (indexed, no vertex normals): a floor quad, a low back
         wall and a row of PATCHES small upright patches, one material each.  Mesh 1: one plain patch with vertex normals whose shading
         normal faces away from its geometry (the only surface of the stage that faces away from the sun).  The stage is open: most
         paths leave it, so a hostile value reaches a minority of the pixels.
  box    24 x 24, the closed inward-facing box of test_gpu_shadow_skip.dark_box_scene with one material per face and an emissive quad
         inside; its light is below and outside.  Paths live past the reference's Russian-roulette depth (4).
Material sets (SETS) and lights (LIGHTS) are the edges of
  emissive.x != 0               -0.0 and (0, 5, 5) do not emit; 1e-45, NaN and (-2, 1, .5) do
  std::max(0.05f, 1 - |beta|)   diffuse 0 (q = 1), |beta| = 0.95 ((1, 1, 1) * K95) and 1 (K1) at the first bounce, beta growing, negative, NaN, inf
  std::max(dot(L, n), 0.0f)     a NaN dot (a NaN vertex normal), 0 * inf, NaN and negative intensities, a zero direction
  the shadow-skip rule          non-finite intensities and betas on surfaces that face away from the light

Two classes (test_hostile_shade_cpu.py asserts the split):
  FIXTURE  reference-defined: no refraction material, and no specular material under a directional or environment light.  Stored with
           the compiled reference's image (8 spp, seed 12345) and ray counts in tests/golden/hostile_shade.npz by tests/golden/make_golden.py.
  PRODUCT  product-defined, compared with the live oracle only: a refraction material (it scatters along a zero direction in every
           bounce: a counted ray that misses; include/prt_hip.h, DESIGN.md "Documented deviations") at a first hit and on the box face
           behind the camera, which only a bounce reaches; specular patches under the hostile suns."""
import os

import numpy as np

import prt_testlib as T

F = np.float32
GOLDEN_FILE = os.path.join(T.GOLDEN, "hostile_shade.npz")
SPP, SEED = 8, 12345
PATCHES = 9
NAN, INF = float("nan"), float("inf")
PLAIN = (0.7, 0.6, 0.5)
STAGE_CAMERA = ((0.0, 1.3, 3.2), (0.0, -0.3, -1.0), 32, 32)
BOX_CAMERA = ((0.0, 0.0, 0.9), (0.0, -0.2, -1.0), 24, 24)


def _exact_k(target):
    """A float32 k near target / sqrt(3) with sqrt(k*k + k*k + k*k) == target in float32, every operation rounded."""
    k = F(target) / np.sqrt(F(3.0))
    lo = hi = k
    for _ in range(64):
        for c in (lo, hi):
            kk = F(c * c)
            if np.sqrt(F(F(kk + kk) + kk)) == F(target):
                return float(c)
        lo, hi = np.nextafter(lo, F(0)), np.nextafter(hi, F(2))
    raise AssertionError(target)


K95 = _exact_k(0.95)
K1 = (0.0, 1.0, 0.0)  # no float32 k gives sqrt(3 k^2) == 1; this length is 1 exactly, so q = max(0.05, 0)


def _m(kd=PLAIN, ke=(0.0, 0.0, 0.0), refl=0):
    kd = (kd, kd, kd) if np.isscalar(kd) else kd
    return (tuple(kd), tuple(ke), refl)


P = _m()
LAMP = _m((0.5, 0.5, 0.5), (1.0, 0.8, 0.6))
_EMIT = [_m(0.5, e) for e in ((-0.0, 5.0, 5.0), (0.0, 5.0, 5.0), (1e-45, 0.0, 0.0), (-2.0, 1.0, 0.5), (NAN, 0.0, 0.0), (INF, 1.0, 1.0), (1.0, NAN, 1.0))]
# PATCHES materials per set, left to right
SETS = {
    "plain": [P] * PATCHES,
    "rr": [_m(0.0), _m(1.0), _m((3.0, 2.0, 1.5)), _m(1e-30), _m((-0.5, 0.5, 0.5)), _m(1e30), _m(K95), _m(K1), P],
    "emit": _EMIT + [P, P],
    "nonfinite": [P, _m((NAN, 0.5, 0.5)), P, _m((INF, 0.5, 0.5)), P, _m((0.8, -INF, 0.8)), P, _m(1e30), P],
    "emit_spec": _EMIT + [_m(0.9, (2.0, 2.0, 2.0), refl=1), _m(0.9, refl=1)],
    "rr_refract": [_m(0.0), _m(1.0), _m((3.0, 2.0, 1.5)), _m(1e-30), _m((-0.5, 0.5, 0.5)), _m(1e30), _m(K95), _m(K1), _m(0.5, (1.0, 2.0, 3.0), refl=2)],
    "rr_spec": [_m(0.0), _m(1.0), _m((3.0, 2.0, 1.5)), _m(1e-30, refl=1), _m((-0.5, 0.5, 0.5)), _m(1e30, refl=1), _m(K95), _m(0.9, (0.0, 5.0, 5.0), refl=1),
                _m(0.9, refl=1)],
}
SUN_DIR = tuple(float(v) for v in (np.array([0.3, 1.0, 0.6]) / np.linalg.norm([0.3, 1.0, 0.6])).astype(F))
SUN = (SUN_DIR, (3.0, 2.5, 2.0))
LIGHTS = {
    "sun": SUN,
    "zero": ((0.0, 0.0, 0.0), SUN[1]),              # the occlusion ray has a zero direction; the dot product is 0
    "unnorm": ((2.0, 9.0, 3.0), SUN[1]),            # an unnormalised direction scales the addend and the ray's origin
    "neg": (SUN_DIR, (-3.0, 2.5, -0.0)),            # negative pixels
    "nan": (SUN_DIR, (3.0, NAN, 2.0)),
    "inf_below": ((0.0, -1.0, 0.0), (INF, 1.0, 1.0)),  # max(dot, 0) = 0 everywhere: 0 * inf
}
# name -> (material set, floor and wall material, light name or None, environment light)
STAGES = {
    "plain": ("plain", P, "sun", False),  # what the scene-edit tests start from
    "rr": ("rr", P, "sun", False),
    "emit": ("emit", P, "sun", False),
    "nonfinite": ("nonfinite", P, "sun", False),
    "light_zero": ("rr", LAMP, "zero", False),              # the lamp floor and wall: without them every value is zero or NaN
    "light_unnorm": ("rr", P, "unnorm", False),
    "light_neg": ("rr", P, "neg", False),
    "light_nan": ("rr", P, "nan", False),
    "light_inf_below": ("rr", LAMP, "inf_below", False),
    "nan_normal": ("rr", P, "sun", False),                # mesh 1 has a NaN vertex normal: a NaN dot product, which std::max(dot, 0.0f) keeps
    "nolight_spec": ("emit_spec", LAMP, None, False),     # specular patches, one of them emissive, where no light makes them undefined
    "rr_sky": ("rr", P, None, True),
    "nonfinite_sky": ("nonfinite", P, None, True),
    "refract_first": ("rr_refract", P, "sun", False),
    "spec_light_nan": ("rr_spec", P, "nan", False),
    "spec_light_inf_below": ("rr_spec", LAMP, "inf_below", False),
    "spec_light_neg": ("rr_spec", P, "neg", False),
}
QUAD = _m(0.5, (4.0, 3.0, 2.0))
# name -> the materials of the faces x = -1, x = 1, y = -1, y = 1, z = -1, z = 1 (behind the camera) and of the inner quad
BOXES = {
    "box_rr": [_m(1.0), _m((3.0, 2.0, 1.5)), _m((-0.5, 0.5, 0.5)), _m(0.8), _m(K95), _m(0.05), QUAD],
    "box_nan": [P, P, P, _m(0.5, (2.0, 2.0, 2.0)), P, P, _m((NAN, 0.5, 0.5))],
    "box_inf": [P, P, P, _m(0.5, (2.0, 2.0, 2.0)), P, P, _m((INF, 0.5, 0.5))],  # an infinite beta meets 0 * I on the faces that look away from the light
    "refract_box": [_m(1.0), _m((3.0, 2.0, 1.5)), _m((-0.5, 0.5, 0.5)), _m(0.8), _m(K95), _m(0.5, (1.0, 1.0, 1.0), refl=2), QUAD],
}
BOX_LIGHT = (tuple(float(v) for v in (np.array([0.2, -1.0, 0.1]) / np.linalg.norm([0.2, -1.0, 0.1])).astype(F)), (16.7, 15.6, 11.7))
FIXTURE = ("rr", "emit", "nonfinite", "light_zero", "light_unnorm", "light_neg", "light_nan", "light_inf_below", "nan_normal", "nolight_spec",
           "rr_sky", "nonfinite_sky", "box_rr", "box_nan", "box_inf")
OTHER = ("plain",)
PRODUCT = ("refract_first", "refract_box", "spec_light_nan", "spec_light_inf_below", "spec_light_neg")


def material_array(mats):
    return np.array([T.make_material(diffuse=kd, emissive=ke, reflection=r) for kd, ke, r in mats], dtype=T.MATERIAL_DTYPE)


def sky():
    return T.sky_env(16, 8)


# ----------------------------------------------------------------------------- geometry
def _quads(quads):
    """(positions (4n, 3), indices (2n, 3)) of quads given by four corners each; the geometric normal is cross(p1 - p0, p2 - p0)."""
    pos = np.array(quads, dtype=F).reshape(-1, 3)
    idx = np.concatenate([[(4 * q, 4 * q + 1, 4 * q + 2), (4 * q, 4 * q + 2, 4 * q + 3)] for q in range(len(quads))]).astype(np.uint32)
    return pos, idx


def stage_geometry():
    """Mesh 0: floor (material 0), wall (1), patch k (2 + k), two triangles each; mesh 1: the patch whose vertex normals are (0, 0, -1)."""
    quads = [[(-3, 0, 3), (3, 0, 3), (3, 0, -2.5), (-3, 0, -2.5)],       # normal +y
             [(-3, 0, -2), (3, 0, -2), (3, 1, -2), (-3, 1, -2)]]         # normal +z; the floor behind it shadows it from below
    for k in range(PATCHES):
        x0 = (k - (PATCHES - 1) / 2) * 0.38 - 0.15
        quads.append([(x0, 0.05, 0), (x0 + 0.3, 0.05, 0), (x0 + 0.3, 0.6, 0), (x0, 0.6, 0)])
    pos, idx = _quads(quads)
    away, aidx = _quads([[(-0.3, 0.75, -0.6), (0.3, 0.75, -0.6), (0.3, 1.15, -0.7), (-0.3, 1.15, -0.7)]])  # (tilted: a mesh whose box has no depth is never hit)
    return (pos, idx, np.repeat(np.arange(len(quads), dtype=np.uint32), 2)), (away, aidx, np.tile(np.array([(0, 0, -1)], dtype=F), (4, 1)))


def box_geometry():
    """test_gpu_shadow_skip.dark_box_scene's box, every face's normal pointing inwards, material = face; an upward quad at y = -0.3."""
    c = np.array([(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=F)  # corner x*4 + y*2 + z
    faces = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    idx = []
    for f in faces:
        p = c[list(f)]
        inward = np.dot(np.cross(p[1] - p[0], p[2] - p[0]), -p.mean(0)) > 0
        a, b, cc, d = f if inward else f[::-1]
        idx += [(a, b, cc), (a, cc, d)]
    q = np.array([(-0.25, -0.3, -0.15), (0.25, -0.3, -0.15), (0.25, -0.3, -0.65), (-0.25, -0.3, -0.65)], dtype=F)
    idx += [(8, 9, 10), (8, 10, 11)]
    return np.concatenate([c, q]), np.array(idx, dtype=np.uint32), np.repeat(np.arange(7, dtype=np.uint32), 2)


# ----------------------------------------------------------------------------- scenes for the product and the oracle
def _mesh(pos, idx, prim_material, mats, normals=None):
    import prt_amd
    m = prt_amd.Mesh.from_arrays(idx, pos, prim_material, material_array(mats).view(prt_amd.MATERIAL_DTYPE), normals=normals)
    m.calculate_bounds()
    return m


def stage_materials(name):
    """The materials of mesh 0 of stage `name`: floor, wall, the patches."""
    mset, wall, _, _ = STAGES[name]
    return [wall, wall] + SETS[mset]


def scene(name, light="own"):
    """(prt_amd.Scene, Camera) of scene `name`; light = a name of LIGHTS replaces the stage's directional light."""
    import prt_amd
    s = prt_amd.Scene()
    if name in BOXES:
        pos, idx, pm = box_geometry()
        s.add(_mesh(pos, idx, pm, BOXES[name]))
        s.set_directional_light(*BOX_LIGHT)
        cam = BOX_CAMERA
    else:
        _, _, own, env = STAGES[name]
        (pos, idx, pm), (apos, aidx, anrm) = stage_geometry()
        s.add(_mesh(pos, idx, pm, stage_materials(name)))
        if name == "nan_normal":
            anrm[2] = np.nan  # both triangles use vertex 2: every normal of the patch is NaN
        s.add(_mesh(apos, aidx, np.zeros(2, np.uint32), [P], normals=anrm))
        light = own if light == "own" else light
        if light is not None:
            s.set_directional_light(*LIGHTS[light])
        if env:
            s.set_infinite_area_light(sky())
        cam = STAGE_CAMERA
    return s, prt_amd.Camera().create(*cam)


def desc(name):
    """T.SceneDesc of scene `name`, the arrays as the product uploads them."""
    s, camera = scene(name)
    d = T.scene_desc_from_product(s, camera, 1.0)
    d.product_scene = s
    return d


def all_materials(d):
    return [m for mesh in d.meshes for m in mesh.materials]


def is_reference_defined(d):
    """No refraction material; no specular material where a light makes the reference read what it never wrote."""
    refl = {int(m["reflectionType"]) for m in all_materials(d)}
    lit = d.light is not None or d.env is not None
    return refl <= {0, 1} and not (1 in refl and lit)


def arrays(d):
    """dict of what the fixture stores of a scene besides the reference's answers."""
    out = {}
    for i, m in enumerate(d.meshes):
        out[f"mesh{i}_indices"] = m.indices
        out[f"mesh{i}_positions"] = m.positions
        out[f"mesh{i}_prim_material"] = m.prim_material
        out[f"mesh{i}_materials"] = m.materials.view(np.uint8).reshape(len(m.materials), -1)
        if m.normals is not None:
            out[f"mesh{i}_normals"] = m.normals
    if d.light is not None:
        out["light"] = np.array([d.light[0], d.light[1]], dtype=F)
    if d.env is not None:
        out["env"] = d.env
    return out


def generate():
    """{scene + "/" + key: array} of every FIXTURE scene."""
    out = {}
    for name in FIXTURE:
        d = desc(name)
        assert is_reference_defined(d), name
        assert d.env is None or (np.isfinite(d.env).all() and (d.env >= 0).all()), name
        out.update({f"{name}/{k}": v for k, v in arrays(d).items()})
    return out


# ----------------------------------------------------------------------------- the fixture
_golden = None


def golden_file():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN_FILE))
    return _golden


def golden(name):
    """dict(desc = T.SceneDesc from the STORED arrays, image (h, w, 3), rays = (raysTraced, occludedTraced)) of a FIXTURE scene."""
    z = {k.split("/", 1)[1]: v for k, v in golden_file().items() if k.startswith(name + "/")}
    meshes = []
    for i in range(sum(k.endswith("_indices") for k in z)):
        meshes.append(T.MeshDesc(z[f"mesh{i}_indices"], z[f"mesh{i}_positions"], z[f"mesh{i}_prim_material"],
                                 np.ascontiguousarray(z[f"mesh{i}_materials"]).view(T.MATERIAL_DTYPE).reshape(-1), normals=z.get(f"mesh{i}_normals")))
    pos, direction, w, h = BOX_CAMERA if name in BOXES else STAGE_CAMERA
    light = (z["light"][0], z["light"][1]) if "light" in z else None
    d = T.SceneDesc(meshes, pos, direction, w, h, light=light, env=z.get("env"))
    return dict(desc=d, image=z["ref_image"], rays=tuple(int(v) for v in z["ref_rays"]))


def first_hit_pixels(d):
    """Pixels whose G-buffer ray (one jittered ray per pixel) first hits each material: {(mesh, material): count}, from the oracle's
    diffuse G-buffer of a copy of the scene whose diffuse colours number the materials."""
    meshes, n = [], 0
    for m in d.meshes:
        mats = m.materials.copy()
        mats["diffuse"] = (np.arange(len(mats), dtype=F) + F(n + 1))[:, None]
        mats["diffuseMap"] = -1
        meshes.append(T.MeshDesc(m.indices, m.positions, m.prim_material, mats, normals=m.normals))
        n += len(mats)
    g = T.OracleScene(T.SceneDesc(meshes, d.cam_pos, d.cam_dir, d.width, d.height)).gbuffer(0, (0, 0, d.width - 1, d.height - 1))[..., 0]
    out, n = {}, 0
    for i, m in enumerate(d.meshes):
        for k in range(len(m.materials)):
            out[(i, k)] = int((g == F(n + k + 1)).sum())
        n += len(m.materials)
    return out


def is_hostile(m):
    """A material with a value outside what the rest of the suite uses: diffuse outside [0.05, 1] or emissive outside {0} u [1, 6]."""
    kd, ke = m["diffuse"].astype(np.float64), m["emissive"].astype(np.float64)
    tame_e = (ke == 0) & ~np.signbit(ke) | (ke >= 1) & (ke <= 6)
    return bool(((kd < 0.05) | (kd > 1) | np.isnan(kd)).any() or not tame_e.all() or m["reflectionType"] != 0)
