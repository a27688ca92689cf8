"""prt_amd -- Python host for the MI355X path-tracing hot path.

The product is libprt_hip.so (hand-written HIP kernels for gfx950 + the C++ host classes that
mirror the reference's Scene/Camera/Mesh/Bvh/Image/PathTracer surface).  This module is the thin
Python mirror of that surface over ctypes: same names, same argument meaning, used by the tests,
bench.py and __graft_entry__.  There is no CPU rendering path here: without the HIP library or a
GPU the render calls raise.

Reference citations (file:line under /root/reference/src) are in include/prt_hip.h and prt_host.h.
"""
import ctypes as C
import os

import numpy as np

from . import _build

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libprt_hip.so")


class PrtError(RuntimeError):
    pass


from ._hiprt import DeviceArrays, runtime as hip_runtime  # noqa: E402  (after PrtError, which _hiprt raises)


# ----------------------------------------------------------------------------- C structs (include/prt_hip.h)
class Material(C.Structure):
    _fields_ = [("diffuse", C.c_float * 3), ("emissive", C.c_float * 3), ("reflectionType", C.c_uint32),
                ("alphaTest", C.c_uint32), ("diffuseMap", C.c_int32), ("bumpMap", C.c_int32)]

    DIFFUSE, SPECULAR, REFRACTION = 0, 1, 2

    @classmethod
    def make(cls, diffuse=(0, 0, 0), emissive=(0, 0, 0), reflection=0):
        m = cls()
        m.diffuse[:] = [float(x) for x in diffuse]
        m.emissive[:] = [float(x) for x in emissive]
        m.reflectionType = reflection
        m.alphaTest = 0
        m.diffuseMap = -1
        m.bumpMap = -1
        return m


class BvhNode(C.Structure):
    _fields_ = [("lower", C.c_float * 3), ("upper", C.c_float * 3), ("primOrSecondNodeIndex", C.c_uint32),
                ("triVectorIndex", C.c_uint32), ("primCount", C.c_uint32), ("splitAxis", C.c_uint32)]


class MeshDesc(C.Structure):
    _fields_ = [("nodeCount", C.c_uint32), ("nodes", C.POINTER(BvhNode)), ("primCount", C.c_uint32),
                ("primRemapping", C.POINTER(C.c_uint32)), ("vertexCount", C.c_uint32), ("indices", C.POINTER(C.c_uint32)),
                ("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)), ("texcoords", C.POINTER(C.c_float)),
                ("materialCount", C.c_uint32), ("primMaterial", C.POINTER(C.c_uint32)), ("materials", C.POINTER(Material))]


class TextureDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("component", C.c_int32), ("texels", C.POINTER(C.c_uint8))]


class SceneDesc(C.Structure):
    _fields_ = [("meshCount", C.c_uint32), ("meshes", C.POINTER(MeshDesc)), ("textureCount", C.c_uint32),
                ("textures", C.POINTER(TextureDesc)), ("hasDirectionalLight", C.c_uint32), ("lightDir", C.c_float * 3),
                ("lightIntensity", C.c_float * 3), ("radius", C.c_float),
                ("hasInfiniteAreaLight", C.c_uint32), ("envWidth", C.c_int32), ("envHeight", C.c_int32),
                ("envTexels", C.POINTER(C.c_float)), ("envVerticalP", C.POINTER(C.c_float)), ("envHorizontalP", C.POINTER(C.c_float))]


class CameraDesc(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("dir", C.c_float * 3), ("up", C.c_float * 3), ("right", C.c_float * 3),
                ("width", C.c_uint32), ("height", C.c_uint32), ("invWidth", C.c_float), ("invHeight", C.c_float)]


class RenderParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("maxDepth", C.c_uint32), ("rrDepth", C.c_uint32), ("seed", C.c_uint32),
                ("exposure", C.c_float), ("tileSize", C.c_uint32), ("rank", C.c_uint32), ("nranks", C.c_uint32),
                ("countTraffic", C.c_uint32)]


class HipStats(C.Structure):
    _fields_ = ([(n, C.c_uint64) for n in ("raysTraced", "occludedTraced", "nBox", "nTri", "nHit", "nTap", "nPx")]
                + [("modeBox", C.c_uint64 * 4), ("modeTri", C.c_uint64 * 4), ("modeTap", C.c_uint64 * 4), ("stackOverflow", C.c_uint64),
                   ("kernelMs", C.c_double), ("kernelMsSum", C.c_double), ("kernelLaunches", C.c_uint64)])

    def as_dict(self):
        out = {}
        for n, t in self._fields_:
            v = getattr(self, n)
            out[n] = [int(x) for x in v] if n.startswith("mode") else (float(v) if n.startswith("kernelMs") else int(v))
        return out


class AccumInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("seed", C.c_uint32), ("maxDepth", C.c_uint32), ("rrDepth", C.c_uint32)]


class AdaptiveParams(C.Structure):
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("minSamples", C.c_uint32), ("maxSamples", C.c_uint32)]


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("normalPowerLog2", C.c_uint32), ("sigmaLuminance", C.c_float), ("sigmaAlbedo", C.c_float),
                ("demodulate", C.c_uint32), ("guideSamples", C.c_uint32)]


class TemporalParams(C.Structure):
    _fields_ = [("positionTolerance", C.c_float), ("normalCos", C.c_float), ("maxHistory", C.c_float)]


class MeshUpdate(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("vertexCount", C.c_uint32), ("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
                ("radius", C.c_float)]


class MeshDeform(C.Structure):
    """prt_mesh_deform (include/prt_hip.h "geometry updates from device memory")."""
    _fields_ = [("mesh", C.c_uint32), ("vertexCount", C.c_uint32), ("positions", C.c_void_p), ("normals", C.c_void_p),
                ("normalsMode", C.c_uint32), ("radius", C.c_float)]

    NORMALS_KEEP, NORMALS_GIVEN, NORMALS_RECOMPUTE = 0, 1, 2
    HOST, RADIUS_AUTO = 1, 2


class MeshInfo(C.Structure):
    """prt_mesh_info: the tree readout of prt_hip_mesh_info."""
    _fields_ = [("vertexBox", C.c_float * 6), ("rootBox", C.c_float * 6), ("radius", C.c_float), ("internalArea", C.c_double),
                ("leafArea", C.c_double), ("rootArea", C.c_double), ("sahCost", C.c_double), ("sahCostAtUpload", C.c_double),
                ("internalNodes", C.c_uint32), ("leaves", C.c_uint32)]

    def as_dict(self):
        return dict(vertexBox=np.array(self.vertexBox[:], dtype=np.float32), rootBox=np.array(self.rootBox[:], dtype=np.float32),
                    radius=np.float32(self.radius), internalArea=float(self.internalArea), leafArea=float(self.leafArea),
                    rootArea=float(self.rootArea), sahCost=float(self.sahCost), sahCostAtUpload=float(self.sahCostAtUpload),
                    internalNodes=int(self.internalNodes), leaves=int(self.leaves))


class LightUpdate(C.Structure):
    _fields_ = [("hasDirectionalLight", C.c_uint32), ("lightDir", C.c_float * 3), ("lightIntensity", C.c_float * 3),
                ("envMode", C.c_uint32), ("envWidth", C.c_int32), ("envHeight", C.c_int32), ("envTexels", C.POINTER(C.c_float))]

    ENV_KEEP, ENV_NONE, ENV_REPLACE = 0, 1, 2


class MaterialUpdate(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("material", C.c_uint32), ("value", Material)]


class TextureUpdate(C.Structure):
    _fields_ = [("texture", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("component", C.c_int32),
                ("texels", C.POINTER(C.c_uint8))]


class DisplayParams(C.Structure):
    """prt_display_params (include/prt_hip.h "display transform")."""
    _fields_ = [("tonemap", C.c_uint32), ("transfer", C.c_uint32), ("format", C.c_uint32), ("meter", C.c_uint32), ("gain", C.c_float),
                ("key", C.c_float), ("lowPermille", C.c_uint32), ("highPermille", C.c_uint32), ("minGain", C.c_float), ("maxGain", C.c_float),
                ("adaptRate", C.c_float)]

    RGB8, RGBA8, BGRA8 = 0, 1, 2
    GAMMA22, SRGB = 0, 1

    @classmethod
    def make(cls, tonemap=True, transfer=0, format=0, meter=False, gain=1.0, key=0.18, low_permille=500, high_permille=950,
             min_gain=2.0 ** -10, max_gain=2.0 ** 10, adapt_rate=1.0):
        return cls(int(tonemap), transfer, format, int(meter), gain, key, low_permille, high_permille, min_gain, max_gain, adapt_rate)

    @property
    def bpp(self):
        return 3 if self.format == 0 else 4


class DisplayState(C.Structure):
    """prt_display_state: the adaptation state and the figures of the last metering."""
    _fields_ = [("gain", C.c_float), ("valid", C.c_uint32), ("octaves", C.c_float), ("target", C.c_float), ("metered", C.c_uint64),
                ("ignored", C.c_uint64), ("hist", C.c_uint32 * 256)]

    def as_dict(self):
        return dict(gain=np.float32(self.gain), valid=int(self.valid), octaves=np.float32(self.octaves), target=np.float32(self.target),
                    metered=int(self.metered), ignored=int(self.ignored), hist=np.array(self.hist[:], dtype=np.uint32))


class Hit(C.Structure):
    _fields_ = [("t", C.c_float), ("i", C.c_float), ("j", C.c_float), ("k", C.c_float), ("primId", C.c_uint32),
                ("meshId", C.c_uint32)]


HIT_DTYPE = np.dtype([("t", "<f4"), ("i", "<f4"), ("j", "<f4"), ("k", "<f4"), ("primId", "<u4"), ("meshId", "<u4")])
# prt_ray / prt_surface (include/prt_hip.h "ray queries")
RAY_DTYPE = np.dtype([("org", "<f4", 3), ("tMax", "<f4"), ("dir", "<f4", 3), ("pad", "<u4")])
SURFACE_DTYPE = np.dtype([("P", "<f4", 3), ("t", "<f4"), ("normal", "<f4", 3), ("material", "<u4"), ("shadingNormal", "<f4", 3),
                          ("meshMaterial", "<u4"), ("uv", "<f4", 2), ("primId", "<u4"), ("meshId", "<u4"), ("diffuse", "<f4", 3),
                          ("pad", "<u4")])
QUERY_HOST = 1  # PRT_HIP_QUERY_HOST
# prt_bake_point / prt_bake_sets (include/prt_hip.h "baking")
BAKE_POINT_DTYPE = np.dtype([("P", "<f4", 3), ("bias", "<f4"), ("N", "<f4", 3), ("set", "<u4")])


class BakeSets(C.Structure):
    """prt_bake_sets: dirs (nSets*K*3 floats) and weights (nSets*K*C floats) are device pointers, or host pointers under QUERY_HOST."""
    _fields_ = [("K", C.c_uint32), ("C", C.c_uint32), ("nSets", C.c_uint32), ("reserved", C.c_uint32), ("dirs", C.c_void_p),
                ("weights", C.c_void_p)]


# prt_atlas_mesh / prt_atlas_counts / prt_atlas_point_params (include/prt_hip.h "lightmap atlases")
class AtlasMesh(C.Structure):
    """prt_atlas_mesh: uv (6 * primCount floats: (u, v) of corners 0, 1, 2, mesh order) is a device pointer, or a host pointer under
    QUERY_HOST."""
    _fields_ = [("meshId", C.c_uint32), ("primCount", C.c_uint32), ("uv", C.c_void_p)]


class AtlasCounts(C.Structure):
    _fields_ = [("n", C.c_uint32), ("rejected", C.c_uint32), ("degenerate", C.c_uint32), ("reserved", C.c_uint32), ("pairs", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in ("n", "rejected", "degenerate", "pairs")}


class AtlasPointParams(C.Structure):
    _fields_ = [("bias", C.c_float), ("setTile", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class AtlasFilterParams(C.Structure):
    """prt_atlas_filter_params (include/prt_hip.h "lightmap filter"): sigmaPosition is in texel footprints."""
    _fields_ = [("iterations", C.c_uint32), ("normalPowerLog2", C.c_uint32), ("sigmaLuminance", C.c_float), ("sigmaPosition", C.c_float),
                ("reserved", C.c_uint32 * 4)]

    def __init__(self, iterations=5, normalPowerLog2=5, sigmaLuminance=4.0, sigmaPosition=4.0):
        super().__init__(iterations=iterations, normalPowerLog2=normalPowerLog2, sigmaLuminance=sigmaLuminance, sigmaPosition=sigmaPosition)


# prt_visibility_params (include/prt_hip.h "visibility baking")
VIS_TRIPLE = 1  # PRT_HIP_VIS_TRIPLE


class VisibilityParams(C.Structure):
    """prt_visibility_params: maxDistance > 0 or +inf, in units of the ray's dir; flags VIS_TRIPLE or 0."""
    _fields_ = [("maxDistance", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    def __init__(self, maxDistance=float("inf"), flags=0):
        super().__init__(maxDistance=maxDistance, flags=flags)


# prt_lens_desc (include/prt_hip.h "lens renders")
LENS_PINHOLE, LENS_ORTHO, LENS_EQUIRECT, LENS_FISHEYE = 0, 1, 2, 3
LENS_CENTRE, LENS_ACCUMULATE = 1, 2


class LensDesc(C.Structure):
    """prt_lens_desc: host memory, read before the call returns.  `pass` is a Python keyword: the field is pass_."""
    _fields_ = [("model", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("K", C.c_uint32), ("pass_", C.c_uint32),
                ("jitterSeed", C.c_uint32), ("flags", C.c_uint32), ("bandRows", C.c_uint32),
                ("pos", C.c_float * 3), ("lensRadius", C.c_float), ("fwd", C.c_float * 3), ("focus", C.c_float),
                ("right", C.c_float * 3), ("fov", C.c_float), ("up", C.c_float * 3), ("reserved", C.c_uint32)]

    def copy(self, **fields):
        """A copy of the record with `fields` replaced."""
        d = LensDesc.from_buffer_copy(self)
        for k, v in fields.items():
            setattr(d, k, _f3(v) if k in ("pos", "fwd", "right", "up") else v)
        return d


NODE_DTYPE = np.dtype([("lower", "<f4", 3), ("upper", "<f4", 3), ("primOrSecondNodeIndex", "<u4"),
                       ("triVectorIndex", "<u4"), ("primCount", "<u4"), ("splitAxis", "<u4")])
MATERIAL_DTYPE = np.dtype([("diffuse", "<f4", 3), ("emissive", "<f4", 3), ("reflectionType", "<u4"),
                           ("alphaTest", "<u4"), ("diffuseMap", "<i4"), ("bumpMap", "<i4")])

# every symbol include/prt_hip.h and include/prt_host.h declare
EXPORTS = [
    "prt_hip_device_count", "prt_hip_create", "prt_hip_destroy", "prt_hip_last_error", "prt_hip_source_sha16", "prt_hip_device_info",
    "prt_hip_upload_scene", "prt_hip_set_camera", "prt_hip_render", "prt_hip_render_gbuffer", "prt_hip_download", "prt_hip_framebuffer", "prt_hip_gather",
    "prt_hip_build_bvh", "prt_hip_comm_unique_id", "prt_hip_comm_init", "prt_hip_comm_adopt", "prt_hip_comm_destroy", "prt_hip_gather_rccl", "prt_hip_gather_payload_bytes",
    "prt_hip_get_stats", "prt_hip_accum_reset", "prt_hip_render_accumulate", "prt_hip_accum_resolve", "prt_hip_accum_export",
    "prt_hip_accum_import", "prt_hip_render_adaptive", "prt_hip_accum_error", "prt_hip_accum_export_moments", "prt_hip_accum_import_moments",
    "prt_hip_denoise_set_guides", "prt_hip_denoise_get_guides", "prt_hip_accum_denoise", "prt_hip_denoise_variance",
    "prt_hip_denoise_get_position", "prt_hip_denoise_set_position", "prt_hip_accum_denoise_temporal", "prt_hip_history_reset",
    "prt_hip_history_export", "prt_hip_history_import", "prt_hip_update_meshes",
    "prt_hip_deform_meshes", "prt_hip_get_mesh_vertices", "prt_hip_mesh_info",
    "prt_hip_update_lights", "prt_hip_update_materials", "prt_hip_update_textures",
    "prt_hip_display", "prt_hip_download_display", "prt_hip_display_get_state", "prt_hip_display_reset", "prt_hip_upload",
    "prt_hip_query_nearest", "prt_hip_query_any", "prt_hip_query_surface", "prt_hip_query_get_counts",
    "prt_hip_query_radiance",
    "prt_hip_bake_rays", "prt_hip_bake_reduce", "prt_hip_bake",
    "prt_hip_atlas_rasterize", "prt_hip_atlas_points", "prt_hip_atlas_resolve", "prt_hip_atlas_filter",
    "prt_hip_bake_visibility", "prt_hip_bake_visibility_reduce",
    "prt_hip_lens_rays", "prt_hip_lens_accumulate", "prt_hip_lens_render",
    "prt_host_scene_set_material", "prt_host_scene_set_texture_texels",
    "prt_host_mesh_cornell", "prt_host_mesh_load_obj", "prt_host_mesh_from_arrays", "prt_host_mesh_displaced_sphere",
    "prt_host_mesh_atrium", "prt_host_mesh_destroy", "prt_host_mesh_transform", "prt_host_mesh_calculate_vertex_normals",
    "prt_host_mesh_calculate_bounds", "prt_host_mesh_prim_count", "prt_host_scene_create", "prt_host_scene_destroy",
    "prt_host_scene_add_mesh", "prt_host_scene_set_directional_light", "prt_host_scene_set_env_light", "prt_host_scene_load_env_light", "prt_host_scene_describe", "prt_host_scene_bbox", "prt_host_scene_update_positions", "prt_host_save_exr", "prt_host_save_ppm",
    "prt_host_camera_create", "prt_host_bvh_build", "prt_host_free",
]

# include/prt_hip_test.h: row-level entry points of the TEST build of the library (libprt_hip_test.so); the product does not export them
TEST_EXPORTS = ["prt_hip_trace_rays", "prt_hip_test_leaf", "prt_hip_test_sincos", "prt_hip_test_powf", "prt_hip_test_camera",
                "prt_hip_test_denoise_profile", "prt_hip_test_copy_yardstick", "prt_hip_test_temporal_profile", "prt_hip_test_scene_arrays",
                "prt_hip_test_refit_profile", "prt_hip_test_occlusion_skipped", "prt_hip_test_shading_arrays", "prt_hip_test_env_tables_host",
                "prt_hip_test_edit_profile", "prt_hip_test_display_host", "prt_hip_test_display_profile", "prt_hip_test_taps",
                "prt_hip_test_surface", "prt_hip_test_deform_profile", "prt_hip_test_env_sample", "prt_hip_test_atlas_filter_profile"]
TEST_LIB_PATH = os.path.join(_HERE, "lib", "libprt_hip_test.so")

_lib = None
_test_lib = None


def build(force=False):
    """Compile libprt_hip.so (the product) and libprt_hip_test.so (the same sources plus the row-level test entry points)
    for gfx950 with hipcc, in tree."""
    _build.build_library(force=force, test_entry_points=True)
    return _build.build_library(force=force)


def source_sha16():
    """Hash of the kernel sources in the tree (what a build now would be stamped with)."""
    return _build.source_sha16()


def loaded_source_sha16():
    """Hash of the kernel sources the LOADED library was built from (prt_hip_source_sha16): measurements are stamped with this."""
    return lib().prt_hip_source_sha16().decode()


def lib():
    """Load libprt_hip.so.  Fails loudly when it has not been built: the HIP library IS the product."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH, False)
    return _lib


def test_lib():
    """Load libprt_hip_test.so: the product's sources built with -DPRT_TEST_ENTRY_POINTS (row-level parity tests only)."""
    global _test_lib
    if _test_lib is None:
        _test_lib = _load(TEST_LIB_PATH, True)
    return _test_lib


def _load(path, with_test_entry_points):
    if not os.path.exists(path):
        raise PrtError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950).  prt_amd has no CPU fallback.")
    L = C.CDLL(path)
    vp, f32p, u32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    L.prt_hip_last_error.restype = C.c_char_p
    L.prt_hip_source_sha16.restype = C.c_char_p
    L.prt_hip_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.prt_hip_destroy.argtypes = [vp]
    L.prt_hip_destroy.restype = None
    L.prt_hip_device_info.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]
    L.prt_hip_upload_scene.argtypes = [vp, C.POINTER(SceneDesc)]
    L.prt_hip_set_camera.argtypes = [vp, C.POINTER(CameraDesc)]
    L.prt_hip_render.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RenderParams), vp, vp]
    L.prt_hip_download.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    L.prt_hip_render_gbuffer.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, vp, vp]
    L.prt_hip_gather.argtypes = [C.POINTER(vp), C.c_int, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    L.prt_hip_build_bvh.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, vp, u32p, vp, C.POINTER(C.c_double)]
    L.prt_hip_comm_unique_id.argtypes = [vp]
    L.prt_hip_comm_init.argtypes = [vp, vp, C.c_int, C.c_int]
    L.prt_hip_comm_adopt.argtypes = [vp, vp]
    L.prt_hip_comm_destroy.argtypes = [vp]
    L.prt_hip_gather_rccl.argtypes = [vp, vp, C.c_int, vp]
    L.prt_hip_gather_payload_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.prt_hip_framebuffer.restype = vp
    L.prt_hip_framebuffer.argtypes = [vp]
    L.prt_hip_get_stats.argtypes = [vp, C.POINTER(HipStats)]
    L.prt_hip_accum_reset.argtypes = [vp]
    L.prt_hip_render_accumulate.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RenderParams), vp, vp]
    L.prt_hip_accum_resolve.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, vp, vp]
    L.prt_hip_accum_export.argtypes = [vp, C.POINTER(AccumInfo), vp, vp, vp]
    L.prt_hip_accum_import.argtypes = [vp, C.POINTER(AccumInfo), vp, vp, vp]
    L.prt_hip_render_adaptive.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RenderParams), C.POINTER(AdaptiveParams),
                                          C.POINTER(C.c_uint32), vp, vp]
    L.prt_hip_accum_error.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, vp]
    L.prt_hip_accum_export_moments.argtypes = [vp, vp]
    L.prt_hip_accum_import_moments.argtypes = [vp, vp]
    L.prt_hip_denoise_set_guides.argtypes = [vp, vp, vp]
    L.prt_hip_denoise_get_guides.argtypes = [vp, C.c_uint32, vp, vp]
    L.prt_hip_accum_denoise.argtypes = [vp, C.POINTER(DenoiseParams), C.c_float, vp, vp]
    L.prt_hip_denoise_variance.argtypes = [vp, vp]
    L.prt_hip_denoise_get_position.argtypes = [vp, vp]
    L.prt_hip_denoise_set_position.argtypes = [vp, vp]
    L.prt_hip_accum_denoise_temporal.argtypes = [vp, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.c_float, vp, vp]
    L.prt_hip_history_reset.argtypes = [vp]
    L.prt_hip_history_export.argtypes = [vp, C.c_uint32, C.POINTER(CameraDesc), vp, vp, vp]
    L.prt_hip_history_import.argtypes = [vp, C.POINTER(CameraDesc), vp, vp, vp]
    L.prt_hip_update_meshes.argtypes = [vp, C.c_uint32, C.POINTER(MeshUpdate), vp]
    L.prt_hip_deform_meshes.argtypes = [vp, C.c_uint32, C.POINTER(MeshDeform), C.c_uint32, vp]
    L.prt_hip_get_mesh_vertices.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint32, vp]
    L.prt_hip_mesh_info.argtypes = [vp, C.c_uint32, C.POINTER(MeshInfo)]
    L.prt_hip_update_lights.argtypes = [vp, C.POINTER(LightUpdate), vp]
    L.prt_hip_update_materials.argtypes = [vp, C.c_uint32, C.POINTER(MaterialUpdate), vp]
    L.prt_hip_update_textures.argtypes = [vp, C.c_uint32, C.POINTER(TextureUpdate), vp]
    L.prt_hip_display.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DisplayParams), vp, vp, vp]
    L.prt_hip_download_display.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    L.prt_hip_display_get_state.argtypes = [vp, C.POINTER(DisplayState)]
    L.prt_hip_display_reset.argtypes = [vp]
    L.prt_hip_upload.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    L.prt_hip_query_nearest.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp]
    L.prt_hip_query_any.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint32, vp]
    L.prt_hip_query_surface.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp]
    L.prt_hip_query_get_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.prt_hip_query_radiance.argtypes = [vp, C.c_uint32, vp, C.POINTER(RenderParams), vp, C.c_uint32, vp]
    L.prt_hip_bake_rays.argtypes = [vp, C.c_uint32, vp, C.POINTER(BakeSets), vp, C.c_uint32, vp]
    L.prt_hip_bake_reduce.argtypes = [vp, C.c_uint32, vp, C.POINTER(BakeSets), vp, vp, C.c_uint32, vp]
    L.prt_hip_bake.argtypes = [vp, C.c_uint32, vp, C.POINTER(BakeSets), C.POINTER(RenderParams), vp, C.c_uint32, vp]
    L.prt_hip_atlas_rasterize.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(AtlasMesh), vp, vp, C.POINTER(AtlasCounts), C.c_uint32, vp]
    L.prt_hip_atlas_points.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(AtlasPointParams), vp, C.c_uint32, vp]
    L.prt_hip_atlas_resolve.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp]
    L.prt_hip_atlas_filter.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, C.POINTER(AtlasFilterParams), vp, C.c_uint32, vp]
    L.prt_hip_bake_visibility.argtypes = [vp, C.c_uint32, vp, C.POINTER(BakeSets), C.POINTER(VisibilityParams), vp, vp, C.c_uint32, vp]
    L.prt_hip_bake_visibility_reduce.argtypes = [vp, C.c_uint32, vp, C.POINTER(BakeSets), C.POINTER(VisibilityParams), vp, vp, C.c_uint32, vp]
    L.prt_hip_lens_rays.argtypes = [vp, C.POINTER(LensDesc), C.c_uint32, C.c_uint32, vp, C.c_uint32, vp]
    L.prt_hip_lens_accumulate.argtypes = [vp, C.POINTER(LensDesc), C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp]
    L.prt_hip_lens_render.argtypes = [vp, C.POINTER(LensDesc), C.POINTER(RenderParams), vp, C.c_uint32, vp]
    if with_test_entry_points:
        L.prt_hip_test_display_host.argtypes = [C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DisplayParams),
                                                C.POINTER(DisplayState), vp]
        L.prt_hip_test_atlas_filter_profile.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, C.POINTER(AtlasFilterParams), vp, vp]
        L.prt_hip_test_display_profile.argtypes = [vp, C.POINTER(DisplayParams), C.c_uint32, vp]
        L.prt_hip_test_shading_arrays.argtypes = [vp, C.POINTER(C.c_uint64)] + [vp] * 12
        L.prt_hip_test_env_tables_host.argtypes = [C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
        L.prt_hip_test_edit_profile.argtypes = [vp, C.c_uint32, C.POINTER(TextureUpdate), C.c_uint32, vp]
        L.prt_hip_test_scene_arrays.argtypes = [vp, C.POINTER(C.c_uint64), vp, vp, vp, vp, vp, vp, vp]
        L.prt_hip_test_refit_profile.argtypes = [vp, C.c_uint32, C.POINTER(MeshUpdate), C.c_uint32, vp]
        L.prt_hip_test_deform_profile.argtypes = [vp, C.c_uint32, C.POINTER(MeshDeform), C.c_uint32, C.c_uint32, vp]
        L.prt_hip_trace_rays.argtypes = [vp, C.c_int, C.c_uint32, vp, vp, C.c_float, vp]
        L.prt_hip_test_leaf.argtypes = [vp, C.c_uint32, vp, vp]
        L.prt_hip_test_sincos.argtypes = [vp, C.c_uint32, vp, vp, vp]
        L.prt_hip_test_powf.argtypes = [vp, C.c_uint32, vp, vp]
        L.prt_hip_test_camera.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
        L.prt_hip_test_denoise_profile.argtypes = [vp, C.POINTER(DenoiseParams), C.c_float, vp]
        L.prt_hip_test_copy_yardstick.argtypes = [vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.prt_hip_test_temporal_profile.argtypes = [vp, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.c_float, vp]
        L.prt_hip_test_occlusion_skipped.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.prt_hip_test_taps.argtypes = [vp, C.c_uint32, vp, C.c_int, C.c_uint32, vp]
        L.prt_hip_test_surface.argtypes = [vp, C.c_uint32, vp, C.c_int, C.c_uint32, vp]
        L.prt_hip_test_env_sample.argtypes = [vp, C.c_uint32, vp, vp, C.c_int, C.c_uint32]
    for n in ("prt_host_mesh_cornell", "prt_host_mesh_load_obj", "prt_host_mesh_from_arrays", "prt_host_mesh_displaced_sphere",
              "prt_host_mesh_atrium", "prt_host_scene_create"):
        getattr(L, n).restype = vp
    L.prt_host_mesh_cornell.argtypes = [C.c_int]
    L.prt_host_mesh_load_obj.argtypes = [C.c_char_p, C.POINTER(Material)]
    L.prt_host_mesh_from_arrays.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]
    L.prt_host_mesh_displaced_sphere.argtypes = [C.c_uint32, C.c_float, f32p, C.POINTER(Material), C.c_uint32]
    L.prt_host_mesh_atrium.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_float]
    L.prt_host_mesh_destroy.argtypes = [vp]
    L.prt_host_mesh_destroy.restype = None
    L.prt_host_mesh_transform.argtypes = [vp, C.c_float, f32p]
    L.prt_host_mesh_transform.restype = None
    L.prt_host_mesh_calculate_vertex_normals.argtypes = [vp]
    L.prt_host_mesh_calculate_vertex_normals.restype = None
    L.prt_host_mesh_calculate_bounds.argtypes = [vp]
    L.prt_host_mesh_calculate_bounds.restype = None
    L.prt_host_mesh_prim_count.argtypes = [vp]
    L.prt_host_mesh_prim_count.restype = C.c_uint32
    L.prt_host_scene_destroy.argtypes = [vp]
    L.prt_host_scene_destroy.restype = None
    L.prt_host_scene_add_mesh.argtypes = [vp, vp]
    L.prt_host_scene_set_directional_light.argtypes = [vp, f32p, f32p]
    L.prt_host_scene_set_directional_light.restype = None
    L.prt_host_scene_set_env_light.argtypes = [vp, C.c_int32, C.c_int32, vp]
    L.prt_host_scene_set_env_light.restype = None
    L.prt_host_scene_load_env_light.argtypes = [vp, C.c_char_p]
    L.prt_host_save_exr.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, vp, C.c_int]
    L.prt_host_save_ppm.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, vp, C.c_int]
    L.prt_host_scene_describe.argtypes = [vp]
    L.prt_host_scene_describe.restype = C.POINTER(SceneDesc)
    L.prt_host_scene_bbox.argtypes = [vp, f32p]
    L.prt_host_scene_bbox.restype = None
    L.prt_host_scene_update_positions.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp]
    L.prt_host_scene_set_material.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(Material)]
    L.prt_host_scene_set_texture_texels.argtypes = [vp, C.c_uint32, vp]
    L.prt_host_camera_create.argtypes = [f32p, f32p, C.c_uint32, C.c_uint32, C.POINTER(CameraDesc)]
    L.prt_host_camera_create.restype = None
    L.prt_host_bvh_build.argtypes = [C.c_uint32, vp, vp, C.c_int, C.POINTER(C.POINTER(BvhNode)), u32p, C.POINTER(u32p)]
    L.prt_host_free.argtypes = [vp]
    L.prt_host_free.restype = None
    return L


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _check(rc, what):
    if rc != 0:
        raise PrtError(f"{what} failed ({rc}): {lib().prt_hip_last_error().decode()}")


# ----------------------------------------------------------------------------- host mirror
class Mesh:
    """prt::Mesh (mesh.h:30-105) before it is handed to a Bvh."""

    def __init__(self, handle):
        if not handle:
            raise PrtError("mesh creation failed")
        self._h = handle

    @classmethod
    def cornell_box(cls, box=True):
        return cls(lib().prt_host_mesh_cornell(int(box)))

    @classmethod
    def load_obj(cls, path, material=None):
        return cls(lib().prt_host_mesh_load_obj(os.fsencode(path), C.byref(material) if material is not None else None))

    @classmethod
    def from_arrays(cls, indices, positions, prim_material, materials, normals=None, texcoords=None):
        indices = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        positions = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        prim_material = np.ascontiguousarray(prim_material, dtype=np.uint32)
        materials = np.ascontiguousarray(materials, dtype=MATERIAL_DTYPE)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32)
        t = None if texcoords is None else np.ascontiguousarray(texcoords, dtype=np.float32)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        return cls(lib().prt_host_mesh_from_arrays(len(indices), len(positions), len(materials), p(indices), p(positions), p(n),
                                                   p(t), p(prim_material), p(materials)))

    @classmethod
    def displaced_sphere(cls, target_tris, radius, center, material, seed=1):
        return cls(lib().prt_host_mesh_displaced_sphere(target_tris, radius, _f3(center), C.byref(material), seed))

    @classmethod
    def atrium(cls, target_tris, seed=1, alpha_masked=True, bump_mapped=True, emissive_fraction=0.0):
        return cls(lib().prt_host_mesh_atrium(target_tris, seed, int(alpha_masked), int(bump_mapped), emissive_fraction))

    def transform(self, scale, translate):
        lib().prt_host_mesh_transform(self._h, scale, _f3(translate))

    def calculate_vertex_normals(self):
        lib().prt_host_mesh_calculate_vertex_normals(self._h)

    def calculate_bounds(self):
        lib().prt_host_mesh_calculate_bounds(self._h)

    @property
    def prim_count(self):
        return lib().prt_host_mesh_prim_count(self._h)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().prt_host_mesh_destroy(self._h)
            self._h = None


class Scene:
    """prt::Scene (scene.h:11-73) owning its Bvhs."""

    def __init__(self):
        self._h = lib().prt_host_scene_create()

    def add(self, mesh):
        """Bvh::build(std::move(mesh)) + Scene::add(bvh) (main.cpp:24-26)."""
        _check(lib().prt_host_scene_add_mesh(self._h, mesh._h), "prt_host_scene_add_mesh")
        mesh._h = None

    def set_directional_light(self, direction, intensity):
        lib().prt_host_scene_set_directional_light(self._h, _f3(direction), _f3(intensity))

    def set_infinite_area_light(self, env):
        """Scene::setInfiniteAreaLight (scene.h:42-45): `env` is a path to an OpenEXR file (scan lines; NO / RLE / ZIPS / ZIP) or an RGB PFM file, or a float array (h, w, 4) RGBA, row 0 = top."""
        if isinstance(env, (str, bytes, os.PathLike)):
            _check(lib().prt_host_scene_load_env_light(self._h, os.fsencode(env)), "prt_host_scene_load_env_light")
            return
        e = np.ascontiguousarray(env, dtype=np.float32)
        if e.ndim != 3 or e.shape[2] != 4:
            raise PrtError("environment map must be (height, width, 4) float RGBA")
        lib().prt_host_scene_set_env_light(self._h, e.shape[1], e.shape[0], e.ctypes.data_as(C.c_void_p))

    def describe(self):
        return lib().prt_host_scene_describe(self._h)

    def update_positions(self, mesh, positions, normals=None):
        """Scene::updatePositions: new positions ((V, 3) float32, V unchanged) and optionally new vertex normals (None keeps them) for
        mesh number `mesh`.  The tree keeps its shape and is refitted; bounds and radius are recomputed.  describe() / arrays()
        afterwards describe the updated scene, and PathTracer.update_meshes sends it to the device without a new upload."""
        p = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if n is not None and n.shape != p.shape:
            raise PrtError(f"update_positions: {n.shape[0]} normals for {p.shape[0]} positions")
        _check(lib().prt_host_scene_update_positions(self._h, mesh, len(p), p.ctypes.data_as(C.c_void_p),
                                                     None if n is None else n.ctypes.data_as(C.c_void_p)), "prt_host_scene_update_positions")

    def set_material(self, mesh, material, value):
        """Scene::setMaterial: material `material` of mesh `mesh` takes the fields of `value` (a Material, or one element of a
        MATERIAL_DTYPE array); diffuseMap / bumpMap name textures in describe() order (-1 = none).  PathTracer.update_materials sends
        it to the device without a new upload."""
        if not isinstance(value, Material):
            value = Material.from_buffer_copy(np.asarray(value, dtype=MATERIAL_DTYPE).tobytes())
        _check(lib().prt_host_scene_set_material(self._h, mesh, material, C.byref(value)), "prt_host_scene_set_material")

    def set_texture_texels(self, texture, texels):
        """Scene::setTextureTexels: new bytes ((height, width, component) uint8, size unchanged) for texture `texture` in describe() order."""
        d = self.describe().contents
        if not 0 <= texture < d.textureCount:
            raise PrtError(f"set_texture_texels: the scene has no texture {texture}")
        t = d.textures[texture]
        a = np.ascontiguousarray(texels, dtype=np.uint8)
        if a.size != t.width * t.height * t.component:
            raise PrtError(f"set_texture_texels: {a.size} bytes for a {t.width} x {t.height} x {t.component} texture")
        _check(lib().prt_host_scene_set_texture_texels(self._h, texture, a.ctypes.data_as(C.c_void_p)), "prt_host_scene_set_texture_texels")

    def bbox(self):
        b = (C.c_float * 6)()
        lib().prt_host_scene_bbox(self._h, b)
        return np.array(b[:], dtype=np.float32)

    def arrays(self):
        """numpy copies of everything the descriptor points to (for checkers)."""
        d = self.describe().contents
        out = dict(meshes=[], textures=[], has_light=bool(d.hasDirectionalLight), light_dir=np.array(d.lightDir[:], dtype=np.float32),
                   light_intensity=np.array(d.lightIntensity[:], dtype=np.float32), radius=np.float32(d.radius))
        for i in range(d.meshCount):
            m = d.meshes[i]
            as_np = lambda p, n, dt: np.ctypeslib.as_array(p, shape=(n,)).view(dt).copy()  # noqa: E731
            out["meshes"].append(dict(
                nodes=np.frombuffer(C.string_at(m.nodes, m.nodeCount * C.sizeof(BvhNode)), dtype=NODE_DTYPE).copy(),
                remap=as_np(m.primRemapping, m.primCount, np.uint32),
                indices=as_np(m.indices, m.primCount * 3, np.uint32).reshape(-1, 3),
                positions=as_np(m.positions, m.vertexCount * 3, np.float32).reshape(-1, 3),
                normals=as_np(m.normals, m.vertexCount * 3, np.float32).reshape(-1, 3) if m.normals else None,
                texcoords=as_np(m.texcoords, m.vertexCount * 2, np.float32).reshape(-1, 2) if m.texcoords else None,
                prim_material=as_np(m.primMaterial, m.primCount, np.uint32),
                materials=np.frombuffer(C.string_at(m.materials, m.materialCount * C.sizeof(Material)), dtype=MATERIAL_DTYPE).copy()))
        for i in range(d.textureCount):
            t = d.textures[i]
            out["textures"].append(np.ctypeslib.as_array(t.texels, shape=(t.height, t.width, t.component)).copy())
        out["env"] = None
        if d.hasInfiniteAreaLight:
            w, h = d.envWidth, d.envHeight
            out["env"] = np.ctypeslib.as_array(d.envTexels, shape=(h, w, 4)).copy()
            out["env_vertical"] = np.ctypeslib.as_array(d.envVerticalP, shape=(h,)).copy()
            out["env_horizontal"] = np.ctypeslib.as_array(d.envHorizontalP, shape=(h * w,)).copy()
        return out

    def __del__(self):
        if getattr(self, "_h", None):
            lib().prt_host_scene_destroy(self._h)
            self._h = None


class Camera:
    """prt::Camera (camera.h:14-53)."""

    def __init__(self):
        self.desc = CameraDesc()

    def create(self, pos, direction, width, height):
        self.pos_arg = np.asarray(pos, dtype=np.float32)        # the arguments as given (the basis in desc is derived)
        self.dir_arg = np.asarray(direction, dtype=np.float32)
        lib().prt_host_camera_create(_f3(pos), _f3(direction), width, height, C.byref(self.desc))
        return self

    @property
    def width(self):
        return self.desc.width

    @property
    def height(self):
        return self.desc.height


class PathTracer:
    """prt::PathTracer (path_tracer.h:15-38) bound to one GPU through the C-ABI (include/prt_hip.h)."""

    def __init__(self, device=0, max_depth=14, rr_depth=4, seed=12345, test_entry_points=False):
        """test_entry_points=True binds the TEST build of the library (row-level entry points for the parity tests)."""
        L = self._L = test_lib() if test_entry_points else lib()
        self._row_level = test_entry_points
        self._ctx = C.c_void_p()
        self._chk(L.prt_hip_create(device, C.byref(self._ctx)), "prt_hip_create")
        self.max_depth, self.rr_depth, self.seed = max_depth, rr_depth, seed
        self._device = device
        self._scene = None
        self._camera = None

    def _chk(self, rc, what):
        if rc != 0:
            raise PrtError(f"{what} failed ({rc}): {self._L.prt_hip_last_error().decode()}")

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.prt_hip_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def device_info(self):
        name = C.create_string_buffer(256)
        cus = C.c_int()
        self._chk(self._L.prt_hip_device_info(self._ctx, name, 256, C.byref(cus)), "prt_hip_device_info")
        return name.value.decode(), cus.value

    def upload_scene(self, scene):
        self._chk(self._L.prt_hip_upload_scene(self._ctx, scene.describe()), "prt_hip_upload_scene")
        self._scene = scene

    def update_meshes(self, scene, meshes=None, stream=None, keep_normals=False):
        """prt_hip_update_meshes: send the CURRENT positions (and vertex normals, unless keep_normals) of the scene's meshes `meshes`
        (indices; None = all) and its radius to the device, where the scene was uploaded with the same topology: the viewer's path
        after Scene.update_positions.  Empties the accumulator; a pending temporal record becomes the history."""
        d = scene.describe().contents
        ids = list(range(d.meshCount)) if meshes is None else [int(m) for m in meshes]
        ups = (MeshUpdate * max(len(ids), 1))()
        for k, m in enumerate(ids):
            if not 0 <= m < d.meshCount:
                raise PrtError(f"update_meshes: the scene has no mesh {m}")
            md = d.meshes[m]
            ups[k].mesh, ups[k].vertexCount, ups[k].positions = m, md.vertexCount, md.positions
            ups[k].normals = None if keep_normals else md.normals
            ups[k].radius = d.radius
        self._chk(self._L.prt_hip_update_meshes(self._ctx, len(ids), ups, stream), "prt_hip_update_meshes")
        self._scene = scene

    # ---- geometry updates from device memory (include/prt_hip.h)
    def _deforms(self, updates, host):
        """[(mesh, positions, normals_or_mode), ...] -> (MeshDeform array, the host arrays it points into)."""
        if self._scene is None:
            raise PrtError("deform_meshes: upload a scene first")
        d = self._scene.describe().contents
        ups, keep = (MeshDeform * max(len(updates), 1))(), []

        def pointer(a, count):
            if host:
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.size != 3 * count:
                    raise PrtError(f"deform_meshes: {a.size} floats for {count} vertices")
                keep.append(a)
                return a.ctypes.data
            return int(a.data_ptr()) if hasattr(a, "data_ptr") else int(a)

        for k, (m, positions, normals) in enumerate(updates):
            if not 0 <= m < d.meshCount:
                raise PrtError(f"deform_meshes: the scene has no mesh {m}")
            ups[k].mesh, ups[k].vertexCount = m, d.meshes[m].vertexCount
            ups[k].positions = pointer(positions, ups[k].vertexCount)
            if normals is None or (isinstance(normals, (int, np.integer)) and int(normals) in (0, 2)):  # (a mode, not a pointer)
                ups[k].normalsMode = int(normals or 0)
            else:
                ups[k].normalsMode, ups[k].normals = MeshDeform.NORMALS_GIVEN, pointer(normals, ups[k].vertexCount)
        return ups, keep

    def deform_meshes(self, updates, host=False, radius_auto=True, stream=None):
        """prt_hip_deform_meshes: new vertex positions for meshes of the uploaded scene, read from DEVICE memory on `stream`.  updates =
        [(mesh, positions, normals_or_mode), ...]: positions (and given normals) are integer device pointers or objects with
        data_ptr() (a torch tensor), numpy arrays with host=True; normals_or_mode is MeshDeform.NORMALS_KEEP (or None),
        MeshDeform.NORMALS_RECOMPUTE, or the normals themselves.  radius_auto: the library computes the scene's radius; False keeps
        the current one.  The host Scene is not touched: mesh_vertices + Scene.update_positions bring it in step."""
        ups, keep = self._deforms(updates, host)
        flags = (MeshDeform.HOST if host else 0) | (MeshDeform.RADIUS_AUTO if radius_auto else 0)
        self._chk(self._L.prt_hip_deform_meshes(self._ctx, len(updates), ups, flags, stream), "prt_hip_deform_meshes")

    def mesh_vertices(self, mesh, normals=True):
        """prt_hip_get_mesh_vertices to the host: (positions, normals) of mesh `mesh` as (V, 3) float32 arrays, as the library holds
        them since the mesh's first update; normals=False returns (positions, None)."""
        if self._scene is None:
            raise PrtError("mesh_vertices: upload a scene first")
        d = self._scene.describe().contents
        if not 0 <= mesh < d.meshCount:
            raise PrtError(f"mesh_vertices: the scene has no mesh {mesh}")
        v = d.meshes[mesh].vertexCount
        P = np.zeros((v, 3), np.float32)
        N = np.zeros((v, 3), np.float32) if normals else None
        self._chk(self._L.prt_hip_get_mesh_vertices(self._ctx, mesh, P.ctypes.data_as(C.c_void_p), None if N is None else N.ctypes.data_as(C.c_void_p),
                                                    MeshDeform.HOST, None), "prt_hip_get_mesh_vertices")
        return P, N

    def mesh_info(self, mesh):
        """prt_hip_mesh_info as a dict: vertexBox, rootBox, radius, internalArea, leafArea, rootArea, sahCost, sahCostAtUpload,
        internalNodes, leaves.  sahCost / sahCostAtUpload is what a refit has cost the tree."""
        info = MeshInfo()
        self._chk(self._L.prt_hip_mesh_info(self._ctx, mesh, C.byref(info)), "prt_hip_mesh_info")
        return info.as_dict()

    # ---- scene edits (include/prt_hip.h "scene edits"): lights, materials and texels of the uploaded scene, replaced in place
    def update_lights(self, scene, env=True, stream=None):
        """prt_hip_update_lights: send the Scene's lights as describe() reports them.  env=True replaces the environment light by the
        Scene's (tables built on the device) or removes it when the Scene has none; env=False leaves the device's as it is."""
        d = scene.describe().contents
        u = LightUpdate()
        u.hasDirectionalLight = d.hasDirectionalLight
        u.lightDir[:] = d.lightDir[:]
        u.lightIntensity[:] = d.lightIntensity[:]
        u.envMode = LightUpdate.ENV_KEEP
        if env:
            u.envMode = LightUpdate.ENV_REPLACE if d.hasInfiniteAreaLight else LightUpdate.ENV_NONE
            if d.hasInfiniteAreaLight:
                u.envWidth, u.envHeight, u.envTexels = d.envWidth, d.envHeight, d.envTexels
        self._chk(self._L.prt_hip_update_lights(self._ctx, C.byref(u), stream), "prt_hip_update_lights")
        self._scene = scene

    def update_materials(self, scene, which, stream=None):
        """prt_hip_update_materials: send the CURRENT materials `which` = [(mesh, material), ...] of the Scene (after
        Scene.set_material) to the device."""
        d = scene.describe().contents
        ups = (MaterialUpdate * max(len(which), 1))()
        for k, (m, i) in enumerate(which):
            if not (0 <= m < d.meshCount and 0 <= i < d.meshes[m].materialCount):
                raise PrtError(f"update_materials: the scene has no material {i} of mesh {m}")
            ups[k].mesh, ups[k].material, ups[k].value = m, i, d.meshes[m].materials[i]
        self._chk(self._L.prt_hip_update_materials(self._ctx, len(which), ups, stream), "prt_hip_update_materials")
        self._scene = scene

    def update_textures(self, scene, textures, stream=None):
        """prt_hip_update_textures: send the CURRENT texels of the Scene's textures `textures` (indices in describe() order, after
        Scene.set_texture_texels) to the device."""
        d = scene.describe().contents
        ups = (TextureUpdate * max(len(textures), 1))()
        for k, t in enumerate(textures):
            if not 0 <= t < d.textureCount:
                raise PrtError(f"update_textures: the scene has no texture {t}")
            td = d.textures[t]
            ups[k].texture, ups[k].width, ups[k].height, ups[k].component, ups[k].texels = t, td.width, td.height, td.component, td.texels
        self._chk(self._L.prt_hip_update_textures(self._ctx, len(textures), ups, stream), "prt_hip_update_textures")
        self._scene = scene

    def shading_arrays(self):
        """Test build only: what a scene edit can change on the device, as dict(mats (M, 20) f32, alpha_class (words,) u32, texels
        (bytes,) u8, env_texels (h, w, 4), env_vertical (h,), env_horizontal (h * w,) f32, env_first_x (h,) i32 (empty without an
        environment light), env_first_y, has_light, has_env, light_dir (3,), light_intensity (3,))."""
        self._need_row_level()
        counts = (C.c_uint64 * 5)()
        self._chk(self._L.prt_hip_test_shading_arrays(self._ctx, counts, *([None] * 12)), "prt_hip_test_shading_arrays")
        m, cw, tb, w, h = [int(x) for x in counts]
        out = dict(mats=np.zeros((m, 20), np.float32), alpha_class=np.zeros(cw, np.uint32), texels=np.zeros(tb, np.uint8),
                   env_texels=np.zeros((h, w, 4), np.float32), env_vertical=np.zeros(h, np.float32), env_horizontal=np.zeros(h * w, np.float32),
                   env_first_x=np.zeros(h, np.int32), env_first_y=np.zeros(1, np.int32), has_light=np.zeros(1, np.uint32),
                   light_dir=np.zeros(3, np.float32), light_intensity=np.zeros(3, np.float32), has_env=np.zeros(1, np.uint32))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        self._chk(self._L.prt_hip_test_shading_arrays(self._ctx, counts, *[ptr(out[k]) for k in (
            "mats", "alpha_class", "texels", "env_texels", "env_vertical", "env_horizontal", "env_first_x", "env_first_y", "has_light",
            "light_dir", "light_intensity", "has_env")]), "prt_hip_test_shading_arrays")
        return out

    def scene_arrays(self):
        """Test build only: the device scene arrays as dict(wnodes (R, 16), hot (256, 16), tris (S, 9), shade (S, 16), bump (S or 0, 12),
        root_boxes (meshes, 6), radius) of float32."""
        self._need_row_level()
        counts = (C.c_uint64 * 5)()
        self._chk(self._L.prt_hip_test_scene_arrays(self._ctx, counts, None, None, None, None, None, None, None), "prt_hip_test_scene_arrays")
        r, h, s, b, m = [int(x) for x in counts]
        out = dict(wnodes=np.zeros((r, 16), np.float32), hot=np.zeros((h, 16), np.float32), tris=np.zeros((s, 9), np.float32),
                   shade=np.zeros((s, 16), np.float32), bump=np.zeros((b, 12), np.float32), root_boxes=np.zeros((8, 6), np.float32),
                   radius=np.zeros(1, np.float32))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        self._chk(self._L.prt_hip_test_scene_arrays(self._ctx, counts, *[ptr(out[k]) for k in ("wnodes", "hot", "tris", "shade", "bump", "root_boxes",
                                                                                          "radius")]), "prt_hip_test_scene_arrays")
        out["root_boxes"] = out["root_boxes"][:m].copy()
        return out

    def set_camera(self, camera):
        self._chk(self._L.prt_hip_set_camera(self._ctx, C.byref(camera.desc)), "prt_hip_set_camera")
        self._camera = camera

    def params(self, samples, exposure=1.0, rank=0, nranks=1, count_traffic=False, max_depth=None, tile=16):
        p = RenderParams()
        p.samples = samples
        p.maxDepth = self.max_depth if max_depth is None else max_depth
        p.rrDepth = self.rr_depth
        p.seed = self.seed
        p.exposure = exposure
        p.tileSize = tile
        p.rank, p.nranks = rank, nranks
        p.countTraffic = int(count_traffic)
        return p

    def render_async(self, x0, y0, x1, y1, samples, d_rgb=None, stream=None, **kw):
        """PathTracer::TraceBlock on the GPU; d_rgb = device pointer (int) or None for the context framebuffer."""
        p = self.params(samples, **kw)
        self._chk(self._L.prt_hip_render(self._ctx, x0, y0, x1, y1, C.byref(p), d_rgb, stream), "prt_hip_render")

    def trace_block(self, x0, y0, x1, y1, samples, **kw):
        """Render the inclusive rectangle and return it as a (h, w, 3) float32 array."""
        self.render_async(x0, y0, x1, y1, samples, **kw)
        W, H = self._camera.width, self._camera.height
        img = np.zeros((H, W, 3), dtype=np.float32)
        self._download(img, x0, y0, x1, y1)
        self.last_stats = self.stats()  # raises on stack overflow
        return img[y0:y1 + 1, x0:x1 + 1].copy()

    def _download(self, img, x0, y0, x1, y1):
        """prt_hip_download reports an earlier launch's error (watchdog, stack overflow) WITHOUT clearing it -- the C-ABI's rule:
        only prt_hip_get_stats consumes it.  The calls of this class that download also own the frame, so they consume it
        here: the error is raised once and the next render on this tracer starts clean."""
        try:
            self._chk(self._L.prt_hip_download(self._ctx, img.ctypes.data_as(C.c_void_p), x0, y0, x1, y1), "prt_hip_download")
        except PrtError:
            try:
                self.stats()
            except PrtError:
                pass
            raise

    def gbuffer(self, kind, x0=0, y0=0, x1=None, y1=None, exposure=1.0):
        """GbufferVisualizer::TraceBlock (gbuffer_visualizer.cpp:17-51): kind 0 diffuse colour, 1 / 2 bump-mapped normal."""
        W, H = self._camera.width, self._camera.height
        x1 = W - 1 if x1 is None else x1
        y1 = H - 1 if y1 is None else y1
        self._chk(self._L.prt_hip_render_gbuffer(self._ctx, x0, y0, x1, y1, kind, self.seed, exposure, None, None), "prt_hip_render_gbuffer")
        img = np.zeros((H, W, 3), dtype=np.float32)
        self._download(img, x0, y0, x1, y1)
        return img[y0:y1 + 1, x0:x1 + 1].copy()

    def render(self, samples, **kw):
        W, H = self._camera.width, self._camera.height
        return self.trace_block(0, 0, W - 1, H - 1, samples, **kw)

    # ---- progressive rendering (include/prt_hip.h "progressive rendering"): passes resume every pixel from the context's accumulator,
    # and after passes of s1, ..., sk samples the image is bit for bit render(s1 + ... + sk)
    def _rect(self, x0, y0, x1, y1):
        W, H = self._camera.width, self._camera.height
        return x0, y0, W - 1 if x1 is None else x1, H - 1 if y1 is None else y1

    def accumulate_async(self, samples, x0=0, y0=0, x1=None, y1=None, d_rgb=None, stream=None, **kw):
        """One accumulate pass of `samples` (a multiple of 8, 8..2040) over the inclusive rectangle, queued on the GPU."""
        x0, y0, x1, y1 = self._rect(x0, y0, x1, y1)
        p = self.params(samples, **kw)
        self._chk(self._L.prt_hip_render_accumulate(self._ctx, x0, y0, x1, y1, C.byref(p), d_rgb, stream), "prt_hip_render_accumulate")

    def accumulate(self, samples, x0=0, y0=0, x1=None, y1=None, exposure=1.0, rank=0, nranks=1, tile=16, count_traffic=False,
                   max_depth=None):
        """One accumulate pass; returns the rectangle's image -- the mean over every sample its pixels have -- as (h, w, 3) float32
        and sets last_stats (the rays of this pass)."""
        x0, y0, x1, y1 = self._rect(x0, y0, x1, y1)
        self.accumulate_async(samples, x0, y0, x1, y1, exposure=exposure, rank=rank, nranks=nranks, tile=tile, count_traffic=count_traffic,
                              max_depth=max_depth)
        return self._download_rect(x0, y0, x1, y1, stats=True)

    def _download_rect(self, x0, y0, x1, y1, stats):
        W, H = self._camera.width, self._camera.height
        img = np.zeros((H, W, 3), dtype=np.float32)
        self._download(img, x0, y0, x1, y1)
        if stats:
            self.last_stats = self.stats()  # raises on stack overflow
        return img[y0:y1 + 1, x0:x1 + 1].copy()

    def accum_reset(self):
        """Empty the accumulator (set_camera and upload_scene do too)."""
        self._chk(self._L.prt_hip_accum_reset(self._ctx), "prt_hip_accum_reset")

    def accum_resolve(self, exposure=1.0, x0=0, y0=0, x1=None, y1=None):
        """exposure * sum / count of the accumulator (0 where nothing was rendered) without tracing; returns the rectangle."""
        x0, y0, x1, y1 = self._rect(x0, y0, x1, y1)
        self._chk(self._L.prt_hip_accum_resolve(self._ctx, x0, y0, x1, y1, exposure, None, None), "prt_hip_accum_resolve")
        return self._download_rect(x0, y0, x1, y1, stats=False)

    def accum_export(self):
        """Checkpoint: dict(width, height, seed, max_depth, rr_depth, rng (H, W) u32, sum (H, W, 3) f32, count (H, W) u32)."""
        W, H = self._camera.width, self._camera.height
        info = AccumInfo()
        rng = np.zeros((H, W), dtype=np.uint32)
        total = np.zeros((H, W, 3), dtype=np.float32)
        count = np.zeros((H, W), dtype=np.uint32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        self._chk(self._L.prt_hip_accum_export(self._ctx, C.byref(info), ptr(rng), ptr(total), ptr(count)), "prt_hip_accum_export")
        return dict(width=info.width, height=info.height, seed=info.seed, max_depth=info.maxDepth, rr_depth=info.rrDepth,
                    rng=rng, sum=total, count=count)

    def accum_import(self, state):
        """Resume: load a dict made by accum_export into this context (same camera size; upload the same scene and camera first)."""
        info = AccumInfo(int(state["width"]), int(state["height"]), int(state["seed"]), int(state["max_depth"]), int(state["rr_depth"]))
        n = info.width * info.height
        rng = np.ascontiguousarray(state["rng"], dtype=np.uint32).reshape(-1)
        total = np.ascontiguousarray(state["sum"], dtype=np.float32).reshape(-1)
        count = np.ascontiguousarray(state["count"], dtype=np.uint32).reshape(-1)
        if len(rng) != n or len(total) != 3 * n or len(count) != n:
            raise PrtError(f"accum_import: arrays do not match the {info.width}x{info.height} accumulator they claim to be")
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        self._chk(self._L.prt_hip_accum_import(self._ctx, C.byref(info), ptr(rng), ptr(total), ptr(count)), "prt_hip_accum_import")

    def accum_counts(self):
        """(H, W) uint32: samples each pixel has in the accumulator."""
        return self.accum_export()["count"]

    def render_progressive(self, total, step=8, budget_ms=None, callback=None, exposure=1.0, **kw):
        """The viewer's loop: accumulate passes of `step` samples over the whole image, calling callback(image, samples_so_far) after
        each, until `total` samples or `budget_ms` of kernel time.  Starts from an empty accumulator; returns (image, samples_reached)."""
        if total < step or total % 8 or step % 8:
            raise PrtError("render_progressive: total and step must be multiples of 8 with total >= step")
        self.accum_reset()
        done, spent, img = 0, 0.0, None
        while done < total:
            n = min(step, total - done)
            img = self.accumulate(n, exposure=exposure, **kw)
            done += n
            spent += self.last_stats["kernelMsSum"]
            if callback is not None:
                callback(img, done)
            if budget_ms is not None and spent >= budget_ms:  # checked after each pass: the first one always runs
                break
        return img, done

    # ---- adaptive sampling (include/prt_hip.h "adaptive sampling"): passes trace only the pixels whose relative standard error is
    # above a threshold; every pixel still holds, bit for bit, the one-shot render of its own sample count
    def adaptive_pass_async(self, samples, threshold, min_spp, max_spp, floor=0.01, x0=0, y0=0, x1=None, y1=None, d_rgb=None, stream=None,
                            **kw):
        """One adaptive pass over the inclusive rectangle: selection, then one launch over the active pixels.  Returns the number of
        active pixels (it waits for the selection, not for the launch)."""
        x0, y0, x1, y1 = self._rect(x0, y0, x1, y1)
        p = self.params(samples, **kw)
        a = AdaptiveParams(threshold, floor, min_spp, max_spp)
        active = C.c_uint32()
        self._chk(self._L.prt_hip_render_adaptive(self._ctx, x0, y0, x1, y1, C.byref(p), C.byref(a), C.byref(active), d_rgb, stream),
                  "prt_hip_render_adaptive")
        return active.value

    def adaptive_pass(self, samples, threshold, min_spp, max_spp, floor=0.01, x0=0, y0=0, x1=None, y1=None, exposure=1.0, rank=0, nranks=1,
                      tile=16, count_traffic=False, max_depth=None):
        """One adaptive pass; returns (the rectangle's image, active pixels) and sets last_stats (this pass's rays; nPx = active).
        Converged pixels are resolved from the accumulator, so the image is that of every pixel's own sample count."""
        x0, y0, x1, y1 = self._rect(x0, y0, x1, y1)
        active = self.adaptive_pass_async(samples, threshold, min_spp, max_spp, floor, x0, y0, x1, y1, exposure=exposure, rank=rank,
                                          nranks=nranks, tile=tile, count_traffic=count_traffic, max_depth=max_depth)
        return self._download_rect(x0, y0, x1, y1, stats=True), active

    def render_adaptive(self, threshold, min_spp=32, max_spp=1024, step=16, floor=0.01, budget_ms=None, callback=None, exposure=1.0, **kw):
        """The adaptive viewer's loop: from an empty accumulator, adaptive passes of `step` samples over the whole image, calling
        callback(image, active) after each, until a pass has no active pixel or `budget_ms` of kernel time is spent.  Returns
        (image, per-pixel sample counts)."""
        self.accum_reset()
        spent, img = 0.0, None
        while True:
            img, active = self.adaptive_pass(step, threshold, min_spp, max_spp, floor, exposure=exposure, **kw)
            spent += self.last_stats["kernelMsSum"]
            if callback is not None:
                callback(img, active)
            if active == 0 or (budget_ms is not None and spent >= budget_ms):  # checked after each pass: the first one always runs
                break
        return img, self.accum_counts()

    def accum_error(self, exposure=1.0, floor=0.01, x0=0, y0=0, x1=None, y1=None):
        """(h, w) float32: the relative standard error of every pixel of the rectangle at this exposure (+inf below two packets)."""
        x0, y0, x1, y1 = self._rect(x0, y0, x1, y1)
        W, H = self._camera.width, self._camera.height
        err = np.zeros((H, W), dtype=np.float32)
        self._chk(self._L.prt_hip_accum_error(self._ctx, x0, y0, x1, y1, exposure, floor, err.ctypes.data_as(C.c_void_p)), "prt_hip_accum_error")
        return err[y0:y1 + 1, x0:x1 + 1].copy()

    def accum_export_moments(self):
        """(H, W, 4) float32: every pixel's moment record {mean, M2, bits(m), 0} (m = [..., 2].view(uint32), packets of 8 samples)."""
        W, H = self._camera.width, self._camera.height
        mom = np.zeros((H, W, 4), dtype=np.float32)
        self._chk(self._L.prt_hip_accum_export_moments(self._ctx, mom.ctypes.data_as(C.c_void_p)), "prt_hip_accum_export_moments")
        return mom

    def accum_import_moments(self, mom):
        """Resume the moments of a checkpoint (after accum_import, which zeroes them): an array made by accum_export_moments."""
        W, H = self._camera.width, self._camera.height
        a = np.ascontiguousarray(mom, dtype=np.float32).reshape(-1)
        if len(a) != 4 * W * H:
            raise PrtError(f"accum_import_moments: {len(a)} floats do not match the camera's {W}x{H} pixels (4 per pixel)")
        self._chk(self._L.prt_hip_accum_import_moments(self._ctx, a.ctypes.data_as(C.c_void_p)), "prt_hip_accum_import_moments")

    # ---- denoised previews (include/prt_hip.h "denoised previews"): an a-trous filter over the accumulator's image, guided by first-hit
    # albedo and normal and by the variance of the moments; it reads the accumulator and changes nothing
    @staticmethod
    def denoise_params(iterations=5, normal_power_log2=5, sigma_luminance=4.0, sigma_albedo=0.1, demodulate=True, guide_samples=8):
        return DenoiseParams(iterations, normal_power_log2, sigma_luminance, sigma_albedo, int(demodulate), guide_samples)

    def denoise_async(self, iterations=5, normal_power_log2=5, sigma_luminance=4.0, sigma_albedo=0.1, demodulate=True, guide_samples=8,
                      exposure=1.0, d_rgb=None, stream=None):
        """Queue the filter over the whole image; d_rgb = device pointer (int) or None for the context's framebuffer."""
        p = self.denoise_params(iterations, normal_power_log2, sigma_luminance, sigma_albedo, demodulate, guide_samples)
        self._chk(self._L.prt_hip_accum_denoise(self._ctx, C.byref(p), exposure, d_rgb, stream), "prt_hip_accum_denoise")

    def denoise(self, iterations=5, normal_power_log2=5, sigma_luminance=4.0, sigma_albedo=0.1, demodulate=True, guide_samples=8,
                exposure=1.0):
        """The denoised image of the accumulator as (H, W, 3) float32 (+0 where nothing was rendered)."""
        self.denoise_async(iterations, normal_power_log2, sigma_luminance, sigma_albedo, demodulate, guide_samples, exposure)
        W, H = self._camera.width, self._camera.height
        return self._download_rect(0, 0, W - 1, H - 1, stats=False)

    def denoise_guides(self, guide_samples=8):
        """(albedo, normal), each (H, W, 3) float32: the guide planes a denoise with this guide_samples uses (rendered if stale; the
        host's own if set_denoise_guides set them)."""
        W, H = self._camera.width, self._camera.height
        albedo = np.zeros((H, W, 3), dtype=np.float32)
        normal = np.zeros((H, W, 3), dtype=np.float32)
        self._chk(self._L.prt_hip_denoise_get_guides(self._ctx, guide_samples, albedo.ctypes.data_as(C.c_void_p),
                                                     normal.ctypes.data_as(C.c_void_p)), "prt_hip_denoise_get_guides")
        return albedo, normal

    def set_denoise_guides(self, albedo, normal):
        """Supply the guide planes ((H, W, 3) each: albedo, and the normal as 0.5*n + 0.5 with (0, 0, 0) for a miss); None, None returns
        to the library's own."""
        if albedo is None and normal is None:
            self._chk(self._L.prt_hip_denoise_set_guides(self._ctx, None, None), "prt_hip_denoise_set_guides")
            return
        if albedo is None or normal is None:
            raise PrtError("set_denoise_guides: both planes or neither")
        W, H = self._camera.width, self._camera.height
        a = np.ascontiguousarray(albedo, dtype=np.float32)
        n = np.ascontiguousarray(normal, dtype=np.float32)
        if a.shape != (H, W, 3) or n.shape != (H, W, 3):
            raise PrtError(f"set_denoise_guides: planes of shape {a.shape} and {n.shape} do not match the camera's ({H}, {W}, 3)")
        self._chk(self._L.prt_hip_denoise_set_guides(self._ctx, a.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p)),
                  "prt_hip_denoise_set_guides")

    def denoise_variance(self):
        """(H, W) float32: the filtered variance V_final of the last denoise (-1 where unknown or nothing was rendered)."""
        W, H = self._camera.width, self._camera.height
        var = np.zeros((H, W), dtype=np.float32)
        self._chk(self._L.prt_hip_denoise_variance(self._ctx, var.ctypes.data_as(C.c_void_p)), "prt_hip_denoise_variance")
        return var

    # ---- temporal reprojection (include/prt_hip.h "temporal reprojection"): the denoiser with the previous view's result merged in
    # wherever the same surface is still visible; set_camera promotes the last temporal denoise of a view to the history
    @staticmethod
    def temporal_params(position_tolerance=0.01, normal_cos=0.9, max_history=256.0):
        return TemporalParams(position_tolerance, normal_cos, max_history)

    def denoise_temporal_async(self, position_tolerance=0.01, normal_cos=0.9, max_history=256.0, iterations=5, normal_power_log2=5,
                               sigma_luminance=4.0, sigma_albedo=0.1, demodulate=True, guide_samples=8, exposure=1.0, d_rgb=None,
                               stream=None):
        """Queue the temporal stage and the filter over the whole image; d_rgb / stream as in denoise_async."""
        p = self.denoise_params(iterations, normal_power_log2, sigma_luminance, sigma_albedo, demodulate, guide_samples)
        t = self.temporal_params(position_tolerance, normal_cos, max_history)
        self._chk(self._L.prt_hip_accum_denoise_temporal(self._ctx, C.byref(p), C.byref(t), exposure, d_rgb, stream),
                  "prt_hip_accum_denoise_temporal")

    def denoise_temporal(self, position_tolerance=0.01, normal_cos=0.9, max_history=256.0, iterations=5, normal_power_log2=5,
                         sigma_luminance=4.0, sigma_albedo=0.1, demodulate=True, guide_samples=8, exposure=1.0):
        """The denoised image of the accumulator merged with the history, as (H, W, 3) float32; this view's result becomes the
        pending record, which the next set_camera of the same size promotes to the history."""
        self.denoise_temporal_async(position_tolerance, normal_cos, max_history, iterations, normal_power_log2, sigma_luminance,
                                    sigma_albedo, demodulate, guide_samples, exposure)
        W, H = self._camera.width, self._camera.height
        return self._download_rect(0, 0, W - 1, H - 1, stats=False)

    def denoise_position(self):
        """(H, W, 4) float32 {X.xyz, t}: the first-hit position guide of the current view ({0, 0, 0, -1} for a miss); rendered if
        stale, the host's own if set_denoise_position set it."""
        W, H = self._camera.width, self._camera.height
        pos = np.zeros((H, W, 4), dtype=np.float32)
        self._chk(self._L.prt_hip_denoise_get_position(self._ctx, pos.ctypes.data_as(C.c_void_p)), "prt_hip_denoise_get_position")
        return pos

    def set_denoise_position(self, position):
        """Supply the position plane ((H, W, 4): {X.xyz, t}, t < 0 for a miss); None returns to the library's own."""
        if position is None:
            self._chk(self._L.prt_hip_denoise_set_position(self._ctx, None), "prt_hip_denoise_set_position")
            return
        W, H = self._camera.width, self._camera.height
        a = np.ascontiguousarray(position, dtype=np.float32)
        if a.shape != (H, W, 4):
            raise PrtError(f"set_denoise_position: a plane of shape {a.shape} does not match the camera's ({H}, {W}, 4)")
        self._chk(self._L.prt_hip_denoise_set_position(self._ctx, a.ctypes.data_as(C.c_void_p)), "prt_hip_denoise_set_position")

    def history_reset(self):
        """Drop the history and the pending record."""
        self._chk(self._L.prt_hip_history_reset(self._ctx), "prt_hip_history_reset")

    def history_export(self, which=0):
        """which 0 = history, 1 = pending: dict(camera=CameraDesc, color_var, pos_len, normal), planes (H, W, 4) float32
        ({hC, hV}, {hX, hLen}, {hN, 0}); raises when there is none."""
        W, H = self._camera.width, self._camera.height
        cam = CameraDesc()
        planes = [np.zeros((H, W, 4), dtype=np.float32) for _ in range(3)]
        self._chk(self._L.prt_hip_history_export(self._ctx, which, C.byref(cam), *[p.ctypes.data_as(C.c_void_p) for p in planes]),
                  "prt_hip_history_export")
        return dict(camera=cam, color_var=planes[0], pos_len=planes[1], normal=planes[2])

    def history_import(self, record):
        """Make a record of history_export the history (its size must be the current camera's)."""
        W, H = self._camera.width, self._camera.height
        planes = [np.ascontiguousarray(record[k], dtype=np.float32) for k in ("color_var", "pos_len", "normal")]
        cam = record["camera"]
        if (cam.width, cam.height) == (W, H) and any(p.shape != (H, W, 4) for p in planes):
            raise PrtError(f"history_import: planes of shape {[p.shape for p in planes]} do not match the camera's ({H}, {W}, 4)")
        self._chk(self._L.prt_hip_history_import(self._ctx, C.byref(cam), *[p.ctypes.data_as(C.c_void_p) for p in planes]),
                  "prt_hip_history_import")

    # ---- display transform (include/prt_hip.h "display transform"): the float image as 8-bit display pixels, under a manual gain or a
    # metered exposure that adapts over the frames; it reads the image and changes nothing else in the context
    def upload_image(self, rgb, x0=0, y0=0, x1=None, y1=None):
        """prt_hip_upload: the rectangle of a host image ((H, W, 3) float32 of the camera's size) into the context's framebuffer."""
        W, H = self._camera.width, self._camera.height
        a = np.ascontiguousarray(rgb, dtype=np.float32)
        if a.shape != (H, W, 3):
            raise PrtError(f"upload_image: an image of shape {a.shape} does not match the camera's ({H}, {W}, 3)")
        x0, y0, x1, y1 = self._rect(x0, y0, x1, y1)
        self._chk(self._L.prt_hip_upload(self._ctx, a.ctypes.data_as(C.c_void_p), x0, y0, x1, y1), "prt_hip_upload")

    def display_async(self, params=None, x0=0, y0=0, x1=None, y1=None, d_rgb=None, d_out=None, stream=None):
        """Queue prt_hip_display over the inclusive rectangle: d_rgb / d_out = device pointers (int) or None for the context's
        framebuffer / display buffer; params = a DisplayParams (None: DisplayParams.make())."""
        p = DisplayParams.make() if params is None else params
        x0, y0, x1, y1 = self._rect(x0, y0, x1, y1)
        self._chk(self._L.prt_hip_display(self._ctx, x0, y0, x1, y1, C.byref(p), d_rgb, d_out, stream), "prt_hip_display")

    def display(self, params=None, x0=0, y0=0, x1=None, y1=None):
        """The rectangle of the context's framebuffer as display pixels: (h, w, bpp) uint8."""
        p = DisplayParams.make() if params is None else params
        x0, y0, x1, y1 = self._rect(x0, y0, x1, y1)
        self.display_async(p, x0, y0, x1, y1)
        W, H = self._camera.width, self._camera.height
        out = np.zeros((H, W, p.bpp), dtype=np.uint8)
        self._chk(self._L.prt_hip_download_display(self._ctx, out.ctypes.data_as(C.c_void_p), x0, y0, x1, y1), "prt_hip_download_display")
        return out[y0:y1 + 1, x0:x1 + 1].copy()

    def display_state(self):
        """The adaptation state and the last metering's figures (DisplayState.as_dict)."""
        st = DisplayState()
        self._chk(self._L.prt_hip_display_get_state(self._ctx, C.byref(st)), "prt_hip_display_get_state")
        return st.as_dict()

    def display_reset(self):
        """The next metered display jumps to its target."""
        self._chk(self._L.prt_hip_display_reset(self._ctx), "prt_hip_display_reset")

    # ---- ray queries (include/prt_hip.h "ray queries"): nearest hit, any hit and surface records for batches of the caller's own rays;
    # they read the scene and change nothing else in the context
    def query_nearest_async(self, n, d_rays, d_hits, d_surfaces=None, stream=None):
        """Queue prt_hip_query_nearest on device arrays: d_rays (n prt_ray, 16-byte aligned), d_hits (n prt_hit), d_surfaces (n
        prt_surface, 16-byte aligned, or None) are device pointers (int)."""
        self._chk(self._L.prt_hip_query_nearest(self._ctx, n, d_rays, d_hits, d_surfaces, 0, stream), "prt_hip_query_nearest")

    def query_any_async(self, n, d_rays, d_occluded, stream=None):
        """Queue prt_hip_query_any on device arrays: d_occluded gets one byte 0 / 1 per ray."""
        self._chk(self._L.prt_hip_query_any(self._ctx, n, d_rays, d_occluded, 0, stream), "prt_hip_query_any")

    def query_surface_async(self, n, d_rays, d_hits, d_surfaces, stream=None):
        """Queue prt_hip_query_surface on device arrays: the surface records of the caller's hits (primId in mesh order)."""
        self._chk(self._L.prt_hip_query_surface(self._ctx, n, d_rays, d_hits, d_surfaces, 0, stream), "prt_hip_query_surface")

    def query_nearest(self, org, dir, t_max, surface=False):
        """The nearest hit of every ray: org, dir (n, 3) float32, t_max a scalar or (n,).  Returns hits (n,) HIT_DTYPE (t = -1 for a
        miss; primId in mesh order), and with surface=True (hits, surfaces (n,) SURFACE_DTYPE)."""
        rays = make_rays(org, dir, t_max)
        hits = np.zeros(len(rays), dtype=HIT_DTYPE)
        surf = np.zeros(len(rays), dtype=SURFACE_DTYPE) if surface else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        self._chk(self._L.prt_hip_query_nearest(self._ctx, len(rays), ptr(rays), ptr(hits), ptr(surf), QUERY_HOST, None), "prt_hip_query_nearest")
        return (hits, surf) if surface else hits

    def query_any(self, org, dir, t_max):
        """(n,) uint8: 1 where anything lies on the ray below t_max."""
        rays = make_rays(org, dir, t_max)
        occ = np.zeros(len(rays), dtype=np.uint8)
        self._chk(self._L.prt_hip_query_any(self._ctx, len(rays), rays.ctypes.data_as(C.c_void_p), occ.ctypes.data_as(C.c_void_p), QUERY_HOST, None),
                  "prt_hip_query_any")
        return occ

    def query_surface(self, org, dir, hits):
        """(n,) SURFACE_DTYPE: the surface records of the given hits ((n,) HIT_DTYPE, primId in mesh order) on rays org, dir.  A hit
        with t = -1 or NaN, or with an index outside the scene, gives the miss record (query_get_counts counts the latter)."""
        h = np.ascontiguousarray(hits, dtype=HIT_DTYPE).reshape(-1)
        rays = make_rays(org, dir, 0.0)
        if len(h) != len(rays):
            raise PrtError(f"query_surface: {len(h)} hits for {len(rays)} rays")
        surf = np.zeros(len(rays), dtype=SURFACE_DTYPE)
        self._chk(self._L.prt_hip_query_surface(self._ctx, len(rays), rays.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p),
                                                surf.ctypes.data_as(C.c_void_p), QUERY_HOST, None), "prt_hip_query_surface")
        return surf

    def query_get_counts(self):
        """Records of the last query_surface that failed the range check on the device."""
        n = C.c_uint64()
        self._chk(self._L.prt_hip_query_get_counts(self._ctx, C.byref(n)), "prt_hip_query_get_counts")
        return int(n.value)

    def _probe_params(self, spp, seed, exposure, max_depth):
        p = self.params(spp, exposure=1.0 if exposure is None else exposure, max_depth=max_depth)
        if seed is not None:
            p.seed = seed
        return p

    def query_radiance_async(self, n, d_rays, d_radiance, spp, seed=None, exposure=None, max_depth=None, stream=None):
        """Queue prt_hip_query_radiance on device arrays: d_rays (n prt_ray, 16-byte aligned), d_radiance (3 * n float32) are device
        pointers (int).  Probe q is traced under seed + q (seed None: the tracer's); max_depth / rr_depth are the tracer's."""
        p = self._probe_params(spp, seed, exposure, max_depth)
        self._chk(self._L.prt_hip_query_radiance(self._ctx, n, d_rays, C.byref(p), d_radiance, 0, stream), "prt_hip_query_radiance")

    def query_radiance(self, org, dir, spp, seed=None, exposure=None, max_depth=None):
        """The path-traced radiance arriving along every ray: org, dir (n, 3) float32 (dir as it is: not normalised), spp a multiple
        of 8 from 8 to 2040.  Returns (n, 3) float32 = exposure * colour / spp, probe q being pixel (0, 0) of a 1 x 1 camera at
        org[q] looking along dir[q] under seed + q; sets last_stats (nPx = n).  Needs a scene and no camera."""
        rays = make_rays(org, dir, 0.0)
        out = np.zeros((len(rays), 3), dtype=np.float32)
        p = self._probe_params(spp, seed, exposure, max_depth)
        self._chk(self._L.prt_hip_query_radiance(self._ctx, len(rays), rays.ctypes.data_as(C.c_void_p), C.byref(p),
                                                 out.ctypes.data_as(C.c_void_p), QUERY_HOST, None), "prt_hip_query_radiance")
        self.last_stats = self.stats()  # raises on stack overflow
        return out

    # ---- baking (include/prt_hip.h "baking"): points and direction sets in, weighted radiance sums out
    def bake_async(self, n, d_points, table, d_out, spp, seed=None, exposure=None, max_depth=None, stream=None):
        """Queue prt_hip_bake on device arrays: d_points (n prt_bake_point, 16-byte aligned) and d_out (3 * C * n float32) are device
        pointers (int), table a BakeSets whose dirs and weights are device pointers.  Ray i*K + k is traced under seed + i*K + k."""
        p = self._probe_params(spp, seed, exposure, max_depth)
        self._chk(self._L.prt_hip_bake(self._ctx, n, d_points, C.byref(table), C.byref(p), d_out, 0, stream), "prt_hip_bake")

    def bake(self, points, normals, dirs, weights, spp, bias=1e-4, sets=None, seed=None, exposure=None, max_depth=None):
        """The weighted radiance sums of n points: points, normals (n, 3) float32 (a zero normal: the identity frame), dirs (K, 3) or
        (nSets, K, 3) local directions with z along the normal, weights (K,), (K, C) or (nSets, K, C), sets None or (n,) the set of
        each point.  Returns (n, C, 3) float32: out[i, c] = sum over k of weights[set, k, c] * radiance along ray i*K + k, the rays
        and sums as include/prt_hip.h "baking" defines them; sets last_stats (nPx = n * K).  Needs a scene and no camera."""
        pts = make_bake_points(points, normals, bias, sets)
        d, w, table = make_bake_sets(dirs, weights)
        out = np.zeros((len(pts), table.C, 3), dtype=np.float32)
        p = self._probe_params(spp, seed, exposure, max_depth)
        self._chk(self._L.prt_hip_bake(self._ctx, len(pts), pts.ctypes.data_as(C.c_void_p), C.byref(table), C.byref(p),
                                       out.ctypes.data_as(C.c_void_p), QUERY_HOST, None), "prt_hip_bake")
        self.last_stats = self.stats()  # raises on stack overflow
        return out

    def bake_rays(self, points, normals, dirs, bias=1e-4, sets=None):
        """(n * K,) RAY_DTYPE: the rays bake() traces for these points and directions (prt_hip_bake_rays; needs no scene)."""
        pts = make_bake_points(points, normals, bias, sets)
        d, _, table = make_bake_sets(dirs, None)
        rays = np.zeros(len(pts) * table.K, dtype=RAY_DTYPE)
        self._chk(self._L.prt_hip_bake_rays(self._ctx, len(pts), pts.ctypes.data_as(C.c_void_p), C.byref(table),
                                            rays.ctypes.data_as(C.c_void_p), QUERY_HOST, None), "prt_hip_bake_rays")
        return rays

    def bake_reduce(self, weights, radiance, sets=None):
        """(n, C, 3) float32: bake()'s sums of per-ray radiance the caller kept -- radiance (n, K, 3) float32, weights (K,), (K, C) or
        (nSets, K, C) -- under other weights, without tracing again (prt_hip_bake_reduce)."""
        L = np.ascontiguousarray(radiance, dtype=np.float32)
        if L.ndim != 3 or L.shape[2] != 3:
            raise PrtError(f"bake_reduce: radiance must be (n, K, 3), not {L.shape}")
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.ndim < 3:
            w = w.reshape(1, L.shape[1], -1)
        _, w, table = make_bake_sets(None, w)
        if table.K != L.shape[1]:
            raise PrtError(f"bake_reduce: weights for {table.K} directions, radiance for {L.shape[1]}")
        pts = make_bake_points(np.zeros((len(L), 3), np.float32), np.zeros((len(L), 3), np.float32), 0.0, sets)
        out = np.zeros((len(L), table.C, 3), dtype=np.float32)
        self._chk(self._L.prt_hip_bake_reduce(self._ctx, len(L), pts.ctypes.data_as(C.c_void_p), C.byref(table), L.ctypes.data_as(C.c_void_p),
                                              out.ctypes.data_as(C.c_void_p), QUERY_HOST, None), "prt_hip_bake_reduce")
        return out

    # ---- lens renders (include/prt_hip.h "lens renders"): a camera record in, an image of radiance sums out
    def lens_rays(self, lens, y0=0, y1=None):
        """((y1 - y0) * W * K,) RAY_DTYPE: the rays render_lens() traces for rows [y0, y1) of `lens` (a LensDesc), ray
        ((y - y0)*W + x)*K + k of pixel (x, y) (prt_hip_lens_rays; needs no scene)."""
        y1 = lens.height if y1 is None else y1
        rays = np.zeros(max(y1 - y0, 0) * lens.width * lens.K, dtype=RAY_DTYPE)
        self._chk(self._L.prt_hip_lens_rays(self._ctx, C.byref(lens), y0, y1, rays.ctypes.data_as(C.c_void_p), QUERY_HOST, None),
                  "prt_hip_lens_rays")
        return rays

    def lens_accumulate(self, lens, radiance, image=None, y0=0, y1=None):
        """(H, W, 3) float32: the K radiances of every pixel of rows [y0, y1) summed in order -- radiance ((y1 - y0) * W * K, 3) float32
        -- into `image` (None: zeros), added to what it holds when lens.flags has LENS_ACCUMULATE and written otherwise; the other
        rows stay (prt_hip_lens_accumulate; needs no scene).  `image` itself is not changed."""
        y1 = lens.height if y1 is None else y1
        L = np.ascontiguousarray(radiance, dtype=np.float32).reshape(-1, 3)
        if len(L) != max(y1 - y0, 0) * lens.width * lens.K:
            raise PrtError(f"lens_accumulate: {len(L)} radiances for {max(y1 - y0, 0) * lens.width * lens.K} rays")
        img = np.zeros((lens.height, lens.width, 3), dtype=np.float32) if image is None else \
            np.array(image, dtype=np.float32, order="C").reshape(lens.height, lens.width, 3)
        self._chk(self._L.prt_hip_lens_accumulate(self._ctx, C.byref(lens), y0, y1, L.ctypes.data_as(C.c_void_p),
                                                  img.ctypes.data_as(C.c_void_p), QUERY_HOST, None), "prt_hip_lens_accumulate")
        return img

    def render_lens_async(self, lens, d_image, spp, seed=None, exposure=None, max_depth=None, stream=None):
        """Queue prt_hip_lens_render on device memory: d_image (3 * W * H float32) is a device pointer (int), written, or added to
        when lens.flags has LENS_ACCUMULATE.  One pass: lens.pass_ picks the K rays of every pixel and the probe seeds."""
        p = self._probe_params(spp, seed, exposure, max_depth)
        self._chk(self._L.prt_hip_lens_render(self._ctx, C.byref(lens), C.byref(p), d_image, 0, stream), "prt_hip_lens_render")

    def render_lens(self, lens, spp, passes=1, seed=None, exposure=None, max_depth=None):
        """(H, W, 3) float32: the mean over passes * K rays per pixel of the radiance along the rays of `lens` (a LensDesc), each ray
        traced with spp samples (a multiple of 8).  Passes lens.pass_ .. lens.pass_ + passes - 1 accumulate on the device; the one
        division by passes * K is made here.  Sets last_stats (the last pass's).  Needs a scene and no camera."""
        p = self._probe_params(spp, seed, exposure, max_depth)
        n = lens.width * lens.height * 3
        with DeviceArrays(self._device) as dev:
            d_image = dev.alloc(n * 4)
            for i in range(passes):
                one = lens.copy(pass_=lens.pass_ + i, flags=(lens.flags | LENS_ACCUMULATE) if i else (lens.flags & ~LENS_ACCUMULATE))
                self._chk(self._L.prt_hip_lens_render(self._ctx, C.byref(one), C.byref(p), d_image, 0, None), "prt_hip_lens_render")
            self.last_stats = self.stats()  # synchronises; raises on stack overflow
            img = np.zeros((lens.height, lens.width, 3), dtype=np.float32)
            dev.download(img, d_image)
        return img / np.float32(passes * lens.K)

    # ---- lightmap atlases (include/prt_hip.h "lightmap atlases"): per-corner lightmap UVs in, a lightmap image out
    def atlas_rasterize_device(self, W, H, d_uvs, prim_counts, d_texels, d_hits, stream=None):
        """prt_hip_atlas_rasterize on device arrays: d_uvs {meshId: device pointer of 6 * primCount float32}, prim_counts {meshId:
        primCount}, d_texels and d_hits device pointers with room for W * H entries.  Synchronous (the one step that is): returns the
        counts as a dict, n = the owned texels."""
        recs = (AtlasMesh * len(d_uvs))(*[AtlasMesh(meshId=m, primCount=prim_counts[m], uv=d_uvs[m]) for m in sorted(d_uvs)])
        counts = AtlasCounts()
        self._chk(self._L.prt_hip_atlas_rasterize(self._ctx, W, H, len(recs), recs, d_texels, d_hits, C.byref(counts), 0, stream),
                  "prt_hip_atlas_rasterize")
        return counts.as_dict()

    def atlas_rasterize(self, uvs_per_mesh, W, H):
        """The texels of a W x H atlas the UV triangles cover: uvs_per_mesh is a list by meshId (None: a mesh with no lightmap) or a
        dict {meshId: uv}, uv (primCount, 3, 2) float32.  Returns (texels (n,) uint32 = y * W + x ascending, hits (n,) HIT_DTYPE with
        t = 0, the owner's barycentrics at the texel centre, primId, meshId; counts dict).  Needs no scene."""
        uvs = _atlas_uvs(uvs_per_mesh)
        recs = (AtlasMesh * len(uvs))(*[AtlasMesh(meshId=m, primCount=len(uv), uv=uv.ctypes.data) for m, uv in sorted(uvs.items())])
        texels, hits, counts = np.zeros(W * H, dtype=np.uint32), np.zeros(W * H, dtype=HIT_DTYPE), AtlasCounts()
        self._chk(self._L.prt_hip_atlas_rasterize(self._ctx, W, H, len(recs), recs, texels.ctypes.data_as(C.c_void_p),
                                                  hits.ctypes.data_as(C.c_void_p), C.byref(counts), QUERY_HOST, None), "prt_hip_atlas_rasterize")
        return texels[:counts.n].copy(), hits[:counts.n].copy(), counts.as_dict()

    def atlas_points_async(self, n, W, d_texels, d_hits, d_points, bias=1e-4, set_tile=1, stream=None):
        """Queue prt_hip_atlas_points on device arrays: d_texels (n uint32), d_hits (n prt_hit), d_points (n prt_bake_point, 16-byte
        aligned) are device pointers (int)."""
        p = AtlasPointParams(bias=bias, setTile=set_tile)
        self._chk(self._L.prt_hip_atlas_points(self._ctx, n, W, d_texels, d_hits, C.byref(p), d_points, 0, stream), "prt_hip_atlas_points")

    def atlas_points(self, texels, hits, W, bias=1e-4, set_tile=1):
        """(n,) BAKE_POINT_DTYPE: the bake points of the hits on the scene as it is now; set = (x % set_tile) + set_tile * (y % set_tile)
        of the texel.  A hit outside the scene gives the all-zero point with set 0xffffffff, which bake() answers with +0."""
        t = np.ascontiguousarray(texels, dtype=np.uint32).reshape(-1)
        h = np.ascontiguousarray(hits, dtype=HIT_DTYPE).reshape(-1)
        if len(t) != len(h):
            raise PrtError(f"atlas_points: {len(t)} texels for {len(h)} hits")
        pts = np.zeros(len(h), dtype=BAKE_POINT_DTYPE)
        p = AtlasPointParams(bias=bias, setTile=set_tile)
        self._chk(self._L.prt_hip_atlas_points(self._ctx, len(h), W, t.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), C.byref(p),
                                               pts.ctypes.data_as(C.c_void_p), QUERY_HOST, None), "prt_hip_atlas_points")
        return pts

    def atlas_resolve_async(self, W, H, n, d_texels, d_values, stride, gutter, d_image, d_mask=None, stream=None):
        """Queue prt_hip_atlas_resolve on device arrays: d_values n * stride float32, d_image W * H * stride float32, d_mask W * H bytes
        or None."""
        self._chk(self._L.prt_hip_atlas_resolve(self._ctx, W, H, n, d_texels, d_values, stride, gutter, d_image, d_mask, 0, stream),
                  "prt_hip_atlas_resolve")

    def atlas_resolve(self, texels, values, W, H, gutter=2):
        """(image (H, W) + values.shape[1:] float32, mask (H, W) uint8): values (n, ...) at their texels, everything else +0, then
        `gutter` dilation passes over the 8-neighbourhood; mask 0 = empty, 1 = a value, g + 1 = filled in pass g."""
        t = np.ascontiguousarray(texels, dtype=np.uint32).reshape(-1)
        v = np.ascontiguousarray(values, dtype=np.float32)
        if v.ndim < 1 or len(v) != len(t):
            raise PrtError(f"atlas_resolve: {len(t)} texels for values {v.shape}")
        stride = int(v.size // max(len(t), 1))
        image, mask = np.zeros((H, W) + v.shape[1:], dtype=np.float32), np.zeros((H, W), dtype=np.uint8)
        self._chk(self._L.prt_hip_atlas_resolve(self._ctx, W, H, len(t), t.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), stride, gutter,
                                                image.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p), QUERY_HOST, None),
                  "prt_hip_atlas_resolve")
        return image, mask

    def atlas_filter_async(self, W, H, n, d_texels, d_points, d_values, stride, d_out, params=None, stream=None):
        """Queue prt_hip_atlas_filter on device arrays: d_texels (n uint32), d_points (n prt_bake_point, 16-byte aligned), d_values and
        d_out (n * stride float32 each, stride = 3 * C, ranges that do not overlap) are device pointers (int)."""
        p = AtlasFilterParams() if params is None else params
        self._chk(self._L.prt_hip_atlas_filter(self._ctx, W, H, n, d_texels, d_points, d_values, stride, C.byref(p), d_out, 0, stream),
                  "prt_hip_atlas_filter")

    def atlas_filter(self, texels, points, values, W, H, params=None):
        """The baked values (n, C, 3) or (n, 3 * C) of the points at their texels, filtered in atlas space by the edge-avoiding a-trous
        filter of include/prt_hip.h "lightmap filter" (params: an AtlasFilterParams; None = its defaults), guided by the points'
        positions and normals: float32 of values' shape.  A point that is not placed (a texel outside the atlas, set 0xffffffff, a
        value, position or normal that is not finite, the later of two points of one texel) keeps its values and is no tap.  Needs
        no scene."""
        t = np.ascontiguousarray(texels, dtype=np.uint32).reshape(-1)
        pts = np.ascontiguousarray(points, dtype=BAKE_POINT_DTYPE).reshape(-1)
        v = np.ascontiguousarray(values, dtype=np.float32)
        if v.ndim < 1 or len(v) != len(t) or len(pts) != len(t):
            raise PrtError(f"atlas_filter: {len(t)} texels for {len(pts)} points and values {v.shape}")
        stride = int(v.size // max(len(t), 1))
        out = np.zeros_like(v)
        p = AtlasFilterParams() if params is None else params
        self._chk(self._L.prt_hip_atlas_filter(self._ctx, W, H, len(t), t.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p),
                                               v.ctypes.data_as(C.c_void_p), stride, C.byref(p), out.ctypes.data_as(C.c_void_p), QUERY_HOST, None),
                  "prt_hip_atlas_filter")
        return out

    def lightmap(self, uvs_per_mesh, W, H, dirs, weights, spp, seed=None, bias=1e-4, set_tile=1, gutter=2, exposure=None, max_depth=None,
                 filter=None):
        """A baked lightmap of the uploaded scene: rasterise the lightmap UVs (uvs_per_mesh as for atlas_rasterize), make a bake point
        per owned texel, bake() them under dirs / weights (as for bake(); a point's set is its texel's place in a set_tile x set_tile
        tile) and resolve with `gutter` dilation passes.  Returns (image (H, W, C, 3) float32, mask (H, W) uint8).  Every array between
        the four calls stays on the device: only the UVs and the table go up and only the image and the mask come down.  More than
        2^24 rays are baked in parts of whole points, part i0 under seed + i0 * K, as include/prt_hip.h "baking" says; sets
        last_atlas_counts and last_stats (of the last part).  filter: an AtlasFilterParams to run atlas_filter_async on the baked values
        before they are resolved (they stay on the device); None = no filter."""
        uvs = _atlas_uvs(uvs_per_mesh)
        d, w, table = make_bake_sets(dirs, weights)
        K, Cc = table.K, table.C
        p = self._probe_params(spp, seed, exposure, max_depth)
        image, mask = np.zeros((H, W, Cc, 3), dtype=np.float32), np.zeros((H, W), dtype=np.uint8)
        with DeviceArrays(self._device) as dev:
            d_uv = {m: dev.upload(uv) for m, uv in uvs.items()}
            d_texels, d_hits = dev.alloc(4 * W * H), dev.alloc(HIT_DTYPE.itemsize * W * H)
            counts = self.atlas_rasterize_device(W, H, d_uv, {m: len(uv) for m, uv in uvs.items()}, d_texels, d_hits)
            self.last_atlas_counts = counts
            n = counts["n"]
            if n == 0:
                return image, mask
            d_points, d_out = dev.alloc(BAKE_POINT_DTYPE.itemsize * n), dev.alloc(12 * Cc * n)
            self.atlas_points_async(n, W, d_texels, d_hits, d_points, bias=bias, set_tile=set_tile)
            table.dirs, table.weights = dev.upload(d), dev.upload(w)
            part = max(1, (1 << 24) // K)
            first_seed = p.seed
            for i0 in range(0, n, part):
                p.seed = (first_seed + i0 * K) & 0xffffffff
                self._chk(self._L.prt_hip_bake(self._ctx, min(part, n - i0), d_points + BAKE_POINT_DTYPE.itemsize * i0, C.byref(table), C.byref(p),
                                               d_out + 12 * Cc * i0, 0, None), "prt_hip_bake")
            if filter is not None:
                d_baked, d_out = d_out, dev.alloc(12 * Cc * n)
                self.atlas_filter_async(W, H, n, d_texels, d_points, d_baked, 3 * Cc, d_out, params=filter)
            d_image, d_mask = dev.alloc(image.nbytes), dev.alloc(mask.nbytes)
            self.atlas_resolve_async(W, H, n, d_texels, d_out, 3 * Cc, gutter, d_image, d_mask)
            self.last_stats = self.stats()  # synchronises the context's stream; raises on stack overflow
            dev.download(image, d_image)
            dev.download(mask, d_mask)
        return image, mask

    # ---- visibility baking (include/prt_hip.h "visibility baking"): points and direction sets in, the weights of the open directions out
    def bake_visibility_async(self, n, d_points, table, d_out, max_distance=float("inf"), triple=False, d_occluded=None, stream=None):
        """Queue prt_hip_bake_visibility on device arrays: d_points (n prt_bake_point, 16-byte aligned), d_out (n * C float32, or
        3 * n * C with triple) and d_occluded (n * K bytes, or None: the context keeps them) are device pointers (int), table a
        BakeSets whose dirs and weights are device pointers."""
        v = VisibilityParams(max_distance, VIS_TRIPLE if triple else 0)
        self._chk(self._L.prt_hip_bake_visibility(self._ctx, n, d_points, C.byref(table), C.byref(v), d_out, d_occluded, 0, stream),
                  "prt_hip_bake_visibility")

    def bake_visibility(self, points, normals, dirs, weights, max_distance=float("inf"), bias=1e-4, sets=None, triple=False, return_bytes=False):
        """The summed weights of the directions that escape, per point: points, normals, dirs, weights, bias and sets as for bake(),
        max_distance the length of every ray in units of its direction.  Returns (n, C) float32, or (n, C, 3) with triple (every
        value three times, the layout of bake()): out[i, c] = sum of weights[set, k, c] over the k whose ray i*K + k meets nothing,
        rays, any-hit rules and sum as include/prt_hip.h "visibility baking" defines them; with return_bytes (out, occluded (n, K)
        uint8).  Sets last_stats (raysTraced = n * K).  Needs a scene and no camera."""
        pts = make_bake_points(points, normals, bias, sets)
        d, w, table = make_bake_sets(dirs, weights)
        out = np.zeros((len(pts), table.C, 3) if triple else (len(pts), table.C), dtype=np.float32)
        occ = np.zeros((len(pts), table.K), dtype=np.uint8) if return_bytes else None
        v = VisibilityParams(max_distance, VIS_TRIPLE if triple else 0)
        self._chk(self._L.prt_hip_bake_visibility(self._ctx, len(pts), pts.ctypes.data_as(C.c_void_p), C.byref(table), C.byref(v),
                                                  out.ctypes.data_as(C.c_void_p), None if occ is None else occ.ctypes.data_as(C.c_void_p),
                                                  QUERY_HOST, None), "prt_hip_bake_visibility")
        self.last_stats = self.stats()  # raises on stack overflow
        return (out, occ) if return_bytes else out

    def bake_visibility_reduce(self, weights, occluded, sets=None, triple=False):
        """(n, C) float32, or (n, C, 3) with triple: bake_visibility()'s sums of occlusion bytes the caller kept -- occluded (n, K) uint8,
        weights (K,), (K, C) or (nSets, K, C) -- under other weights, without tracing again (prt_hip_bake_visibility_reduce; needs no
        scene)."""
        b = np.ascontiguousarray(occluded, dtype=np.uint8)
        if b.ndim != 2:
            raise PrtError(f"bake_visibility_reduce: occluded must be (n, K), not {b.shape}")
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.ndim < 3:
            w = w.reshape(1, b.shape[1], -1)
        _, w, table = make_bake_sets(None, w)
        if table.K != b.shape[1]:
            raise PrtError(f"bake_visibility_reduce: weights for {table.K} directions, bytes for {b.shape[1]}")
        pts = make_bake_points(np.zeros((len(b), 3), np.float32), np.zeros((len(b), 3), np.float32), 0.0, sets)
        out = np.zeros((len(b), table.C, 3) if triple else (len(b), table.C), dtype=np.float32)
        v = VisibilityParams(flags=VIS_TRIPLE if triple else 0)
        self._chk(self._L.prt_hip_bake_visibility_reduce(self._ctx, len(b), pts.ctypes.data_as(C.c_void_p), C.byref(table), C.byref(v),
                                                         b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), QUERY_HOST, None),
                  "prt_hip_bake_visibility_reduce")
        return out

    def lightmap_visibility(self, uvs_per_mesh, W, H, dirs, weights, max_distance=float("inf"), bias=1e-4, set_tile=1, gutter=2, filter=None):
        """A visibility lightmap of the uploaded scene (ambient occlusion, sky visibility, bent normals): lightmap() with
        bake_visibility in the place of bake().  Returns (image (H, W, C) float32, or (H, W, C, 3) when `filter` (an
        AtlasFilterParams) is given, mask (H, W) uint8): the bake then writes every value three times, because atlas_filter wants a
        stride that is a multiple of 3.  Every array between the calls stays on the device; sets last_atlas_counts and last_stats."""
        uvs = _atlas_uvs(uvs_per_mesh)
        d, w, table = make_bake_sets(dirs, weights)
        triple = filter is not None
        stride = table.C * (3 if triple else 1)
        image, mask = np.zeros((H, W, table.C, 3) if triple else (H, W, table.C), dtype=np.float32), np.zeros((H, W), dtype=np.uint8)
        with DeviceArrays(self._device) as dev:
            d_uv = {m: dev.upload(uv) for m, uv in uvs.items()}
            d_texels, d_hits = dev.alloc(4 * W * H), dev.alloc(HIT_DTYPE.itemsize * W * H)
            counts = self.atlas_rasterize_device(W, H, d_uv, {m: len(uv) for m, uv in uvs.items()}, d_texels, d_hits)
            self.last_atlas_counts = counts
            n = counts["n"]
            if n == 0:
                return image, mask
            d_points, d_out = dev.alloc(BAKE_POINT_DTYPE.itemsize * n), dev.alloc(4 * stride * n)
            self.atlas_points_async(n, W, d_texels, d_hits, d_points, bias=bias, set_tile=set_tile)
            table.dirs, table.weights = dev.upload(d), dev.upload(w)
            part = max(1, (1 << 30) // table.K)  # whole points, n*K <= 2^30 per call
            for i0 in range(0, n, part):
                self.bake_visibility_async(min(part, n - i0), d_points + BAKE_POINT_DTYPE.itemsize * i0, table, d_out + 4 * stride * i0,
                                           max_distance=max_distance, triple=triple)
            if triple:
                d_baked, d_out = d_out, dev.alloc(4 * stride * n)
                self.atlas_filter_async(W, H, n, d_texels, d_points, d_baked, stride, d_out, params=filter)
            d_image, d_mask = dev.alloc(image.nbytes), dev.alloc(mask.nbytes)
            self.atlas_resolve_async(W, H, n, d_texels, d_out, stride, gutter, d_image, d_mask)
            self.last_stats = self.stats()  # synchronises the context's stream; raises on stack overflow
            dev.download(image, d_image)
            dev.download(mask, d_mask)
        return image, mask

    def pick(self, x, y):
        """What lies under pixel (x, y) of the current camera: the ray through the pixel's centre (the position guide's ray) ->
        (hit, surface), one element of HIT_DTYPE and of SURFACE_DTYPE; hit["t"] == -1 for the background."""
        if self._camera is None:
            raise PrtError("pick: set a camera first")
        W, H = self._camera.width, self._camera.height
        if not (0 <= x < W and 0 <= y < H):
            raise PrtError(f"pick: pixel ({x}, {y}) outside the {W} x {H} image")
        rays = pixel_centre_rays(self._camera.desc, [x], [y])
        hits, surf = self.query_nearest(rays["org"], rays["dir"], rays["tMax"], surface=True)
        return hits[0], surf[0]

    def build_bvh(self, indices, positions):
        """Bvh::build on the GPU (prt_hip_build_bvh): returns (nodes as NODE_DTYPE array, primRemapping, device ms)."""
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        n = len(idx)
        nodes = np.zeros(2 * n, dtype=NODE_DTYPE)
        remap = np.zeros(n, dtype=np.uint32)
        count, ms = C.c_uint32(), C.c_double()
        self._chk(self._L.prt_hip_build_bvh(self._ctx, n, idx.ctypes.data_as(C.c_void_p), len(pos), pos.ctypes.data_as(C.c_void_p),
                                            nodes.ctypes.data_as(C.c_void_p), C.byref(count), remap.ctypes.data_as(C.c_void_p), C.byref(ms)),
                  "prt_hip_build_bvh")
        return nodes[:count.value].copy(), remap, ms.value

    # ---- multi-process image gather over RCCL (include/prt_hip.h "image gather")
    def comm_init(self, unique_id, rank, nranks):
        """Collective: every rank calls it with rank 0's id (comm_unique_id(), shipped over any host channel)."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._chk(self._L.prt_hip_comm_init(self._ctx, buf, rank, nranks), "prt_hip_comm_init")

    def gather_rccl(self, d_rgb=None, root=0, stream=None):
        """Collective: moves the tiles every rank owns (1/nranks of the image) to `root` and de-interleaves them there."""
        self._chk(self._L.prt_hip_gather_rccl(self._ctx, d_rgb, root, stream), "prt_hip_gather_rccl")

    def gather_payload_bytes(self):
        n = C.c_uint64()
        self._chk(self._L.prt_hip_gather_payload_bytes(self._ctx, C.byref(n)), "prt_hip_gather_payload_bytes")
        return n.value

    def stats(self):
        st = HipStats()
        self._chk(self._L.prt_hip_get_stats(self._ctx, C.byref(st)), "prt_hip_get_stats")
        return st.as_dict()

    # ---- row-level entry points (parity tests; include/prt_hip_test.h, test build of the library only)
    def _need_row_level(self):
        if not self._row_level:
            raise PrtError("row-level entry points exist only in libprt_hip_test.so: PathTracer(test_entry_points=True)")

    def trace_rays(self, mode, org, dirs, max_t):
        self._need_row_level()
        org = np.ascontiguousarray(org, dtype=np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        hits = np.zeros(len(org), dtype=HIT_DTYPE)
        self._chk(self._L.prt_hip_trace_rays(self._ctx, mode, len(org), org.ctypes.data_as(C.c_void_p), dirs.ctypes.data_as(C.c_void_p),
                                        max_t, hits.ctypes.data_as(C.c_void_p)), "prt_hip_trace_rays")
        return hits

    def occlusion_skipped(self):
        """Occlusion rays of the last render that were answered without a walk (part of occludedTraced)."""
        self._need_row_level()
        n = C.c_uint64()
        self._chk(self._L.prt_hip_test_occlusion_skipped(self._ctx, C.byref(n)), "prt_hip_test_occlusion_skipped")
        return int(n.value)

    def test_leaf(self, records):
        self._need_row_level()
        rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 22)
        out = np.zeros((len(rec), 24), dtype=np.float32)
        self._chk(self._L.prt_hip_test_leaf(self._ctx, len(rec), rec.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)), "prt_hip_test_leaf")
        return out

    def test_sincos(self, theta):
        self._need_row_level()
        th = np.ascontiguousarray(theta, dtype=np.float32)
        s, c = np.zeros_like(th), np.zeros_like(th)
        self._chk(self._L.prt_hip_test_sincos(self._ctx, len(th), th.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p),
                                         c.ctypes.data_as(C.c_void_p)), "prt_hip_test_sincos")
        return s, c

    def test_powf(self, x):
        self._need_row_level()
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.zeros_like(x)
        self._chk(self._L.prt_hip_test_powf(self._ctx, len(x), x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)), "prt_hip_test_powf")
        return y

    def test_taps(self, records, counting=False, blocks=0):
        """prt_hip_test_taps: (n, 4) uint32 records {material, u bits, v bits, flags} -> (n, 12) uint32 words."""
        self._need_row_level()
        rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 4)
        out = np.zeros((len(rec), 12), dtype=np.uint32)
        self._chk(self._L.prt_hip_test_taps(self._ctx, len(rec), rec.ctypes.data_as(C.c_void_p), int(counting), blocks,
                                            out.ctypes.data_as(C.c_void_p)), "prt_hip_test_taps")
        return out

    def test_surface(self, records, counting=False, blocks=0):
        """prt_hip_test_surface: (n, 5) uint32 records {mesh, primId, i bits, j bits, k bits} -> (n, 20) uint32 words."""
        self._need_row_level()
        rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 5)
        out = np.zeros((len(rec), 20), dtype=np.uint32)
        self._chk(self._L.prt_hip_test_surface(self._ctx, len(rec), rec.ctypes.data_as(C.c_void_p), int(counting), blocks,
                                               out.ctypes.data_as(C.c_void_p)), "prt_hip_test_surface")
        return out

    def test_env_sample(self, u, counting=False, blocks=0):
        """prt_hip_test_env_sample: (n, 2) float32 draws {u.x, u.y} in [0, 1) -> (n, 8) uint32 words {dir[3], color[3], taps counted, 0}."""
        self._need_row_level()
        u = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 2)
        out = np.zeros((len(u), 8), dtype=np.uint32)
        self._chk(self._L.prt_hip_test_env_sample(self._ctx, len(u), u.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), int(counting),
                                                  blocks), "prt_hip_test_env_sample")
        return out

    def test_camera(self, x, y, state):
        self._need_row_level()
        out = np.zeros(92, dtype=np.float32)
        self._chk(self._L.prt_hip_test_camera(self._ctx, x, y, state, out.ctypes.data_as(C.c_void_p)), "prt_hip_test_camera")
        return out


def env_tables_host(env):
    """Test build only: prt_hip_test_env_tables_host -- the arithmetic of the environment kernels on the host, for an (h, w, 4) float
    RGBA image: (vertical (h,), horizontal (h * w,), first_x (h,) int32, first_y, flags)."""
    e = np.ascontiguousarray(env, dtype=np.float32)
    h, w, _ = e.shape
    v, hor, fx = np.zeros(h, np.float32), np.zeros(h * w, np.float32), np.zeros(h, np.int32)
    fy, flags = C.c_int32(), C.c_uint32()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = test_lib().prt_hip_test_env_tables_host(w, h, ptr(e), ptr(v), ptr(hor), ptr(fx), C.addressof(fy), C.addressof(flags))
    if rc != 0:
        raise PrtError(f"prt_hip_test_env_tables_host failed ({rc}): {test_lib().prt_hip_last_error().decode()}")
    return v, hor, fx, fy.value, flags.value


def display_host(rgb, params=None, state=None, x0=0, y0=0, x1=None, y1=None, out=None):
    """Test build only: prt_hip_test_display_host -- the arithmetic of the display kernels on the host, for an (h, w, 3) float image.
    Returns (the whole (h, w, bpp) uint8 image, of which only the rectangle is written -- into `out` when given -- and the DisplayState
    after the call); `state` (a DisplayState) is the adaptation state going in and is not modified."""
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w, _ = a.shape
    p = DisplayParams.make() if params is None else params
    st = DisplayState()
    if state is not None:
        C.memmove(C.byref(st), C.byref(state), C.sizeof(DisplayState))
    o = np.zeros((h, w, p.bpp), dtype=np.uint8) if out is None else out
    rc = test_lib().prt_hip_test_display_host(w, h, a.ctypes.data_as(C.c_void_p), x0, y0, w - 1 if x1 is None else x1, h - 1 if y1 is None else y1,
                                              C.byref(p), C.byref(st), o.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PrtError(f"prt_hip_test_display_host failed ({rc}): {test_lib().prt_hip_last_error().decode()}")
    return o, st


def device_count():
    return lib().prt_hip_device_count()


# ----------------------------------------------------------------------------- ray queries
def make_rays(org, dir, t_max):
    """(n,) RAY_DTYPE from org, dir (n, 3) and t_max (a scalar or (n,)), all taken as float32."""
    o = np.ascontiguousarray(org, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dir, dtype=np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise PrtError(f"{len(o)} origins for {len(d)} directions")
    rays = np.zeros(len(o), dtype=RAY_DTYPE)
    rays["org"], rays["dir"] = o, d
    rays["tMax"] = np.asarray(t_max, dtype=np.float32)
    return rays


# ----------------------------------------------------------------------------- baking
def make_bake_points(points, normals, bias=1e-4, sets=None):
    """(n,) BAKE_POINT_DTYPE from points, normals (n, 3), bias (a scalar or (n,)) and sets (None = set 0, or (n,) uint32)."""
    P = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    N = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    if len(P) != len(N):
        raise PrtError(f"{len(P)} points for {len(N)} normals")
    pts = np.zeros(len(P), dtype=BAKE_POINT_DTYPE)
    pts["P"], pts["N"] = P, N
    pts["bias"] = np.asarray(bias, dtype=np.float32)
    if sets is not None:
        pts["set"] = np.asarray(sets, dtype=np.uint32)
    return pts


def make_bake_sets(dirs, weights):
    """(dirs (nSets, K, 3) or None, weights (nSets, K, C) or None, BakeSets pointing at the two HOST arrays -- keep them alive) from dirs
    (K, 3) or (nSets, K, 3) and weights (K,), (K, C) or (nSets, K, C); either may be None (bake_reduce reads no directions, bake_rays no
    weights)."""
    d = w = None
    if dirs is not None:
        d = np.ascontiguousarray(dirs, dtype=np.float32)
        d = d.reshape((1,) + d.shape) if d.ndim == 2 else d
        if d.ndim != 3 or d.shape[2] != 3:
            raise PrtError(f"bake: dirs must be (K, 3) or (nSets, K, 3), not {d.shape}")
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.ndim < 3:
            if d is None:
                raise PrtError("bake: weights without dirs must be (nSets, K, C)")
            if w.size % (d.shape[0] * d.shape[1]) == 0:
                w = w.reshape(d.shape[0], d.shape[1], -1)
        if w.ndim != 3 or (d is not None and w.shape[:2] != d.shape[:2]):
            raise PrtError(f"bake: weights {w.shape} do not fit dirs {None if d is None else d.shape}")
    shape = d.shape if d is not None else w.shape
    table = BakeSets(K=shape[1], C=1 if w is None else w.shape[2], nSets=shape[0], reserved=0,
                     dirs=None if d is None else d.ctypes.data, weights=None if w is None else w.ctypes.data)
    return d, w, table


# ----------------------------------------------------------------------------- lens renders
def _lens(model, pos, fwd, right, up, W, H, K=1, lens_radius=0.0, focus=1.0, fov=0.0, jitter_seed=0, flags=0, band_rows=0, pass_=0):
    d = LensDesc(model=model, width=W, height=H, K=K, pass_=pass_, jitterSeed=jitter_seed, flags=flags, bandRows=band_rows,
                 lensRadius=lens_radius, focus=focus, fov=fov, reserved=0)
    d.pos, d.fwd, d.right, d.up = _f3(pos), _f3(fwd), _f3(right), _f3(up)
    return d


def _lens_basis(pos, look_at, up):
    """Unit (fwd, right, up) in float64 of a view from pos towards look_at with `up` roughly upwards (right-handed: right = fwd x up)."""
    f = np.asarray(look_at, np.float64) - np.asarray(pos, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    return f, r, np.cross(r, f)


def lens_pinhole(pos, look_at, up, fov_y, W, H, K=1, lens_radius=0.0, focus=1.0, **kw):
    """A perspective LensDesc: fov_y the full vertical angle in radians, |fwd| = 1 (so `focus` is the distance of the plane in focus
    along the view direction); lens_radius > 0 makes it a thin lens.  kw: jitter_seed, flags, band_rows, pass_."""
    f, r, u = _lens_basis(pos, look_at, up)
    t = np.tan(0.5 * fov_y)
    return _lens(LENS_PINHOLE, pos, f, t * W / H * r, t * u, W, H, K, lens_radius, focus, **kw)


def lens_ortho(pos, look_at, up, half_height, W, H, K=1, **kw):
    """An orthographic LensDesc: the image spans 2 * half_height vertically around pos."""
    f, r, u = _lens_basis(pos, look_at, up)
    return _lens(LENS_ORTHO, pos, f, half_height * W / H * r, half_height * u, W, H, K, **kw)


def lens_equirect(pos, W, H, K=1, fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), **kw):
    """A 360 x 180 degree panorama LensDesc around pos: the image centre looks along fwd, the top row towards up."""
    f, r, u = _lens_basis(pos, np.asarray(pos, np.float64) + np.asarray(fwd, np.float64), up)
    return _lens(LENS_EQUIRECT, pos, f, r, u, W, H, K, **kw)


def lens_fisheye(pos, look_at, up, fov, W, H, K=1, **kw):
    """An equidistant fisheye LensDesc: fov the full angle in radians across the image circle (the ellipse inscribed in the image)."""
    f, r, u = _lens_basis(pos, look_at, up)
    return _lens(LENS_FISHEYE, pos, f, r, u, W, H, K, fov=fov, **kw)


def lens_cube_faces(pos, size, K=1, **kw):
    """Six size x size pinhole LensDesc with a 90 degree basis, in the order +x, -x, +y, -y, +z, -z (fwd, then up as the cube-map
    convention of the graphics APIs has them): a cube map needs no model of its own."""
    faces = [((1, 0, 0), (0, -1, 0)), ((-1, 0, 0), (0, -1, 0)), ((0, 1, 0), (0, 0, 1)), ((0, -1, 0), (0, 0, -1)), ((0, 0, 1), (0, -1, 0)),
             ((0, 0, -1), (0, -1, 0))]
    out = []
    for f, u in faces:
        f, u = np.array(f, np.float64), np.array(u, np.float64)
        out.append(_lens(LENS_PINHOLE, pos, f, np.cross(f, u), u, size, size, K, **kw))
    return out


def lens_from_camera(camera, K=1, **kw):
    """The pinhole LensDesc that frames what prt_hip_render frames for `camera` (a Camera or a CameraDesc).  camera.cpp:54-56 at zero
    jitter aims pixel (x, y) along dir + nx*right + ny*up with nx = 2*(x/W - 0.5)*0.6*aspect and ny = -2*(y/H - 0.5)*0.6; the
    lens aims it along fwd' + a*right' + b*up' with a = 2*(x + 0.5)/W - 1 = 2*(x/W - 0.5) + 1/W and b = -2*(y/H - 0.5) - 1/H.
    With right' = 0.6*aspect*right and up' = 0.6*up the two agree when fwd' = dir - right'/W + up'/H: the last two terms take out
    the half pixel between the two footprints.  Computed in float64 and rounded once."""
    c = getattr(camera, "desc", camera)
    W, H = c.width, c.height
    pos, d, up, right = (np.array(list(getattr(c, k)), dtype=np.float64) for k in ("pos", "dir", "up", "right"))
    r2, u2 = 0.6 * (W / H) * right, 0.6 * up
    return _lens(LENS_PINHOLE, pos, d - r2 / W + u2 / H, r2, u2, W, H, K, **kw)


# ----------------------------------------------------------------------------- lightmap atlases
def _atlas_uvs(uvs_per_mesh):
    """{meshId: (primCount, 3, 2) float32} from a list by meshId (None: no lightmap for that mesh) or a dict."""
    items = uvs_per_mesh.items() if isinstance(uvs_per_mesh, dict) else enumerate(uvs_per_mesh)
    uvs = {}
    for m, uv in items:
        if uv is None:
            continue
        a = np.ascontiguousarray(uv, dtype=np.float32)
        if a.size == 0 or a.size % 6 != 0:
            raise PrtError(f"atlas: the UVs of mesh {m} must be (primCount, 3, 2), not {a.shape}")
        uvs[int(m)] = a.reshape(-1, 3, 2)
    if not uvs:
        raise PrtError("atlas: no mesh has lightmap UVs")
    return uvs


def bake_cosine_set(K, rng):
    """(dirs (K, 3), weights (K, 1)) float32: K cosine-weighted directions about +z (pdf = cos / pi) and weights pi / K, so that
    bake() returns irradiance (C = 1).  rng: a numpy Generator."""
    u1, u2 = rng.random(K), rng.random(K)
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    dirs = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u1)], axis=1).astype(np.float32)
    return dirs, np.full((K, 1), np.pi / K, dtype=np.float32)


def sh9_basis(d):
    """(len(d), 9): the real spherical harmonics of bands 0 to 2 at unit directions d (n, 3), in the order
    1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2."""
    x, y, z = (np.asarray(d, dtype=np.float64)[:, k] for k in range(3))
    return np.stack([0.28209479177387814 * np.ones_like(x), 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
                     1.0925484305920792 * x * y, 1.0925484305920792 * y * z, 0.31539156525252005 * (3.0 * z * z - 1.0),
                     1.0925484305920792 * x * z, 0.5462742152960396 * (x * x - y * y)], axis=1)


def bake_sh9_set(K, rng):
    """(dirs (K, 3), weights (K, 9)) float32: K uniform directions on the sphere and weights 4 pi / K * Y_c(d_k), so that bake() at a
    point with a zero normal returns the SH9 coefficients of the radiance arriving there (C = 9)."""
    z, phi = rng.uniform(-1.0, 1.0, K), rng.uniform(0.0, 2.0 * np.pi, K)
    r = np.sqrt(1.0 - z * z)
    dirs = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)
    return dirs, (4.0 * np.pi / K * sh9_basis(dirs)).astype(np.float32)


def pixel_centre_rays(cam, xs, ys):
    """(n,) RAY_DTYPE: the rays through the centres of pixels (xs[k], ys[k]) of camera `cam` (a CameraDesc) -- the position guide's rays
    (include/prt_hip.h "temporal reprojection": camera_dir with both jitter terms 0.0f, tMax = 100000), operation by operation in float32."""
    F = np.float32
    x = np.asarray(xs, dtype=np.uint32).astype(F)
    y = np.asarray(ys, dtype=np.uint32).astype(F)
    right, up, fwd, pos = (np.array(list(getattr(cam, k)), dtype=F) for k in ("right", "up", "dir", "pos"))
    k_aspect = F(cam.width) / F(cam.height)
    nx = F(2.0) * (x * F(cam.invWidth) - F(0.5) + F(0.0)) * F(0.6) * k_aspect
    ny = F(-2.0) * (y * F(cam.invHeight) - F(0.5) + F(0.0)) * F(0.6)
    v = ((nx[:, None] * right + ny[:, None] * up) + fwd).astype(F)
    inv = F(1.0) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    rays = np.zeros(len(x), dtype=RAY_DTYPE)
    rays["org"] = pos
    rays["dir"] = (inv[:, None] * v).astype(F)
    rays["tMax"] = F(100000.0)
    return rays


# ----------------------------------------------------------------------------- the reference's scene setups (main.cpp:22-105)
def setup_cornell_box(width, height, teapot_obj=None, teapot_mesh=None):
    """setupCornellBox (main.cpp:22-55).  The teapot comes from an OBJ file or from a ready Mesh."""
    scene = Scene()
    scene.add(Mesh.cornell_box(True))
    if teapot_obj is not None:
        teapot_mesh = Mesh.load_obj(teapot_obj, Material.make(diffuse=(0.9, 0.9, 0.9), reflection=Material.SPECULAR))
        teapot_mesh.transform(0.005, (-0.5, 0.0, 0.5))
    if teapot_mesh is not None:
        teapot_mesh.calculate_vertex_normals()
        teapot_mesh.calculate_bounds()
        scene.add(teapot_mesh)
    camera = Camera().create((0, 0.965, 2.6), (0, 0, -1.0), width, height)
    return scene, camera, 1.0


def _normalize(v):
    v = np.asarray(v, dtype=np.float32)
    d = np.float32(v[0] * v[0]) + np.float32(v[1] * v[1]) + np.float32(v[2] * v[2])
    inv = np.float32(1.0) / np.sqrt(np.float32(d), dtype=np.float32)
    return (inv * v).astype(np.float32)


def setup_bunny_standin(width, height, tris=69451, seed=1):
    """BASELINE config 2 stand-in: Cornell box + a bunny-class displaced sphere (69 451 triangles
    asked for; a lat-long grid gives the nearest even count) in place of the teapot, plus the directional light of
    setupSanMiguelLowPoly (main.cpp:84) so that occlusion rays are exercised."""
    scene = Scene()
    scene.add(Mesh.cornell_box(True))
    m = Mesh.displaced_sphere(tris, 0.3, (-0.45, 0.36, 0.45), Material.make(diffuse=(0.8, 0.75, 0.7)), seed)
    m.calculate_vertex_normals()
    m.calculate_bounds()
    scene.add(m)
    scene.set_directional_light(_normalize((0.2, 1.0, 0.2)), (16.7, 15.6, 11.7))
    camera = Camera().create((0, 0.965, 2.6), (0, 0, -1.0), width, height)
    return scene, camera, 1.0


def setup_atrium_standin(width, height, tris=262000, seed=1, alpha=True, bump=True, emissive_fraction=0.0, light=True):
    """BASELINE config 3 stand-in: Sponza-class atrium, light as setupSponza (main.cpp:66)."""
    scene = Scene()
    m = Mesh.atrium(tris, seed, alpha, bump, emissive_fraction)
    m.calculate_vertex_normals()
    scene.add(m)
    if light:
        scene.set_directional_light(_normalize((0.05, 1.0, 0.1)), (16.7, 15.6, 11.7))
    camera = Camera().create((-15.0, 4.0, 0.5), (1.0, 0.08, -0.05), width, height)
    return scene, camera, 1.0


# ----------------------------------------------------------------------------- multi-GPU sharding (one process per GPU)
def owned_pixel_mask(width, height, rank, nranks, tile=16):
    """Boolean (height, width) mask of the pixels rank `rank` renders: 16x16 tiles (main.cpp:123-124) dealt round-robin,
    tile id = ty * tiles_per_row + tx, owner = id % nranks -- the rule prt_hip_render applies on the device."""
    ty, tx = np.meshgrid(np.arange(height) // tile, np.arange(width) // tile, indexing="ij")
    tiles_x = (width + tile - 1) // tile
    return ((ty * tiles_x + tx) % nranks) == rank


def save_exr(path, rgb, zip=True):
    """Image::saveExr (image.cpp:82-139): (H, W, 3) float image -> half-float OpenEXR with channels B, G, R (ZIP blocks like
    tinyexr's default, or raw scan lines)."""
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    _check(lib().prt_host_save_exr(os.fsencode(path), a.shape[1], a.shape[0], a.ctypes.data_as(C.c_void_p), int(zip)), "prt_host_save_exr")


def save_ppm(path, rgb, tonemap=True):
    """Image::savePpm (image.cpp:52-80): c/(c+1) tone map (optional), clamp, gamma 1/2.2, 8 bits."""
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    _check(lib().prt_host_save_ppm(os.fsencode(path), a.shape[1], a.shape[0], a.ctypes.data_as(C.c_void_p), int(tonemap)), "prt_host_save_ppm")


def comm_unique_id():
    """128 bytes naming a new RCCL communicator (rank 0 calls this and broadcasts the bytes)."""
    buf = C.create_string_buffer(128)
    _check(lib().prt_hip_comm_unique_id(buf), "prt_hip_comm_unique_id")
    return buf.raw


def gather_contexts(tracers, x0, y0, x1, y1):
    """prt_hip_gather: one process driving several contexts (tracer i rendered the rectangle with rank=i, nranks=len(tracers)
    into its own framebuffer); returns the assembled (H, W, 3) image."""
    cam = tracers[0]._camera
    img = np.zeros((cam.height, cam.width, 3), dtype=np.float32)
    arr = (C.c_void_p * len(tracers))(*[t._ctx for t in tracers])
    _check(lib().prt_hip_gather(arr, len(tracers), img.ctypes.data_as(C.c_void_p), x0, y0, x1, y1), "prt_hip_gather")
    return img


def owned_tile_ids(width, height, rank, nranks, tile=16):
    """Tile ids rank, rank + nranks, ... of the image's tile grid: the order of the tiles in a rank's packed buffer."""
    total = ((width + tile - 1) // tile) * ((height + tile - 1) // tile)
    return np.arange(rank, total, nranks, dtype=np.int64)


def pack_tiles(image, rank, nranks, tile=16):
    """Host mirror of the library's pack kernel (prt_gather.hip): the tiles `rank` owns, tile-major, (n, tile, tile, 3);
    pixels beyond the image's edge are zero."""
    H, W, _ = image.shape
    tiles_x = (W + tile - 1) // tile
    ids = owned_tile_ids(W, H, rank, nranks, tile)
    out = np.zeros((len(ids), tile, tile, 3), dtype=np.float32)
    for q, t in enumerate(ids):
        x0, y0 = int(t % tiles_x) * tile, int(t // tiles_x) * tile
        crop = image[y0:y0 + tile, x0:x0 + tile]
        out[q, :crop.shape[0], :crop.shape[1]] = crop
    return out


def unpack_tiles(image, packed, rank, nranks, tile=16):
    """Host mirror of the de-interleave kernel: writes rank's packed tiles into `image` (in place)."""
    H, W, _ = image.shape
    tiles_x = (W + tile - 1) // tile
    for q, t in enumerate(owned_tile_ids(W, H, rank, nranks, tile)):
        x0, y0 = int(t % tiles_x) * tile, int(t // tiles_x) * tile
        h, w = min(tile, H - y0), min(tile, W - x0)
        image[y0:y0 + h, x0:x0 + w] = packed[q, :h, :w]
    return image


def gather_image_host(framebuffer, rank, nranks, dst=0, tile=16):
    """The gather's data movement on HOST tensors over torch.distributed point-to-point (gloo in the CPU tests): every rank
    sends the tiles it owns, packed as the device packs them, to `dst`, which de-interleaves them -- the same ownership
    rule, tile order and payload as prt_hip_gather_rccl, without the GPU.  `framebuffer` is a (H, W, 3) float32 numpy array."""
    import torch
    import torch.distributed as dist
    H, W, _ = framebuffer.shape
    if rank != dst:
        mine = pack_tiles(framebuffer, rank, nranks, tile)
        if mine.size:
            dist.send(torch.from_numpy(mine), dst=dst)
        return framebuffer
    for r in range(nranks):
        n = len(owned_tile_ids(W, H, r, nranks, tile))
        if r == dst or n == 0:
            continue
        buf = torch.empty((n, tile, tile, 3), dtype=torch.float32)
        dist.recv(buf, src=r)
        unpack_tiles(framebuffer, buf.numpy(), r, nranks, tile)
    return framebuffer
