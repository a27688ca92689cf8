"""The GPU test kit: the fixtures and helpers the GPU test modules share (a library module like prt_testlib.py, no tests of its own).

Fixtures are defined once here and imported by name into the modules that use them, as
    from prt_gpukit import rows, rows2  # noqa: F401
pytest registers a fixture it finds in a test module's namespace under that module, so scope="module" still means one context per
test module.  A module whose fixture differs in effect keeps its own and says how in a comment.  Helpers that drive a context through
cases several modules share are in prt_gpucases.py."""
import numpy as np
import pytest

import prt_amd
import prt_hostile_shade as HS
import prt_hostile_taps as HT
import prt_denoise_ref as R
import prt_testlib as T
from prt_bake_ref import same_bytes  # noqa: F401  (re-exported: words equal, a NaN where the restatement has one)
from prt_testlib import assert_bits_equal, bits  # noqa: F401  (re-exported)

F = np.float32
U = np.uint32


# ----------------------------------------------------------------------------- fixtures (imported by name into the modules that use them)
@pytest.fixture(scope="module", autouse=True)
def gpu_event_accounting():
    """The oracle's nBox/nTri/nTap for occlusion queries follow the GPU's near-first visit in this module (the images
    and ray counts are the reference traversal's either way; the oracle aborts if the two visits ever disagree)."""
    T.oracle().orc_set_anyhit_accounting(1)
    yield
    T.oracle().orc_set_anyhit_accounting(0)


@pytest.fixture(scope="module")
def tracer():
    prt_amd.build()
    t = prt_amd.PathTracer()
    yield t
    t.close()


@pytest.fixture(scope="module")
def rows():
    """A context of the TEST build of the library (libprt_hip_test.so: the product's sources + the row-level entry points
    of include/prt_hip_test.h).  Whole-image tests run on `tracer`, the product library."""
    prt_amd.build()
    t = prt_amd.PathTracer(test_entry_points=True)
    yield t
    t.close()


@pytest.fixture(scope="module")
def rows2():
    prt_amd.build()
    t = prt_amd.PathTracer(test_entry_points=True)
    yield t
    t.close()


class CheckedArrays(prt_amd.DeviceArrays):
    """prt_amd.DeviceArrays whose every allocation is asserted to be 16-byte aligned (prt_bake_point and prt_ray want that)."""

    def alloc(self, nbytes):
        p = super().alloc(nbytes)
        assert p % 16 == 0, hex(p)
        return p


@pytest.fixture
def dev():
    """Device memory and streams for one test: everything is freed and destroyed when the test ends, passed or not."""
    with CheckedArrays() as d:
        yield d


def fetch(dev, p, count, dtype=U):
    """`count` elements of `dtype` from device address p (a copy on the null stream: behind a context's blocking stream)."""
    out = np.zeros(count, dtype=dtype)
    dev.download(out, p)
    return out


def stage_tracers(scenes, arrays=False, **tracer_kw):
    """A module-scoped `tracers` fixture: tracers(name) is a PathTracer(**tracer_kw) with scenes[name]() uploaded (a Scene, or a tuple
    that starts with one) and no camera, made on first use and closed with the module; "none" is a context without a scene.  With
    arrays=True it returns (context, the scene's mesh arrays or None)."""
    @pytest.fixture(scope="module")
    def tracers():
        prt_amd.build()
        made = {}

        def get(name):
            if name not in made:
                t, meshes = prt_amd.PathTracer(**tracer_kw), None
                if name != "none":
                    scene = scenes[name]()
                    scene = scene[0] if isinstance(scene, tuple) else scene
                    t.upload_scene(scene)
                    meshes = scene.arrays()["meshes"] if arrays else None
                made[name] = (t, meshes)
            return made[name] if arrays else made[name][0]
        yield get
        for t, _ in made.values():
            t.close()
    return tracers


# ----------------------------------------------------------------------------- comparisons
def assert_same_image(img, ref, what):
    """Bit patterns equal; where the oracle has a NaN the GPU must have one too (sign and payload of a NaN differ between SSE and the GPU)."""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(img), nan), f"{what}: NaN pixels differ"
    a = np.ascontiguousarray(img, dtype=np.float32).view(np.uint32)[~nan]
    b = np.ascontiguousarray(ref, dtype=np.float32).view(np.uint32)[~nan]
    bad = np.nonzero(a != b)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} values differ, first at {int(bad[0])}"


# (prt_bake_ref.same_bytes takes words and lets a NaN answer a NaN; this one takes records and wants every byte)
def same_records(got, want, what):
    if got.tobytes() != want.tobytes():
        a, b = got.view(np.uint8).reshape(len(got), -1), want.view(np.uint8).reshape(len(want), -1)
        bad = np.unique(np.nonzero(a != b)[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ, first {bad[:4]}: {got[bad[0]]} != {want[bad[0]]}")


# ----------------------------------------------------------------------------- output arrays and pointers
SENTINEL = 0xffc0bad1   # a NaN no kernel here produces
TAIL = 16               # sentinel words behind every output


def sentinel(words):
    return np.full(words, SENTINEL, dtype=U)


def ptr(a):
    return a if a is None or isinstance(a, int) else a.ctypes.data


# ----------------------------------------------------------------------------- scenes and states
def upload(tracer, scene, camera):
    tracer.upload_scene(scene)
    tracer.set_camera(camera)


def sky_stage():
    """The plain stage lit by prt_hostile_shade.sky() instead of its sun: the ENV instantiation."""
    s, cam = HS.scene("plain", light=None)
    s.set_infinite_area_light(HS.sky())
    return s, cam


SCENES = {"plain": lambda: HS.scene("plain"), "sky": sky_stage, "box_rr": lambda: HS.scene("box_rr")}


@pytest.fixture(scope="module")
def box_scene():
    return prt_amd.setup_cornell_box(64, 64)[0]


def camera_of(width, height):
    return prt_amd.setup_cornell_box(width, height)[1]


@pytest.fixture(scope="module")
def c1_scene():
    return prt_amd.setup_cornell_box(512, 512, teapot_mesh=T.teapot_product_mesh())


def snapped_scene(z, width=64, height=48):
    """The two-quad scene of tests/test_gpu_hostile_taps.py: an alpha-masked quad (primitives 0, 1) in z = 0 and a bump-mapped, textured
    one (primitives 2, 3) in z = -1, seen head-on from (0, 0, 3)."""
    tex = HT.golden_maps(z)
    names = [n for n, _ in tex]
    a, g, c = names.index("b4_16x16"), names.index("g1_3x5"), names.index("n4_3x5")
    mats = np.array([T.make_material(diffuse=(0.9, 0.8, 0.7), alpha_test=1, diffuse_map=a),
                     T.make_material(diffuse=(1.0, 1.0, 1.0), diffuse_map=c, bump_map=g)], dtype=T.MATERIAL_DTYPE)

    def quad(half, zpos, t0, t1):
        pos = np.array([[-half, -half, zpos], [half, -half, zpos], [half, half, zpos], [-half, half, zpos]], dtype=F)
        tc = np.array([[t0, t0], [t1, t0], [t1, t1], [t0, t1]], dtype=F)
        return pos, tc
    p0, t0 = quad(1.0, 0.0, -1.0, 2.0)
    p1, t1 = quad(2.5, -1.0, -2.0 / 3.0, 5.0 / 3.0)
    pos, tc = np.concatenate([p0, p1]), np.concatenate([t0, t1])
    idx = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=np.uint32)
    mesh = T.MeshDesc(idx, pos, np.array([0, 0, 1, 1], dtype=np.uint32), mats, texcoords=tc)
    return T.SceneDesc([mesh], cam_pos=(0.0, 0.0, 3.0), cam_dir=(0.0, 0.0, -1.0), width=width, height=height,
                       light=((0.0, 0.0, 1.0), (3.0, 3.0, 2.5)), textures=[t for _, t in tex])


def synthetic_state(width, height, seed):
    """Random accumulator, moments and guides with every special case of the header in them: count 0, m < 2, miss normals, zero
    variance, albedo 0, radiance from 1e-6 to 1e3 (HDR emitters next to dark walls)."""
    rng = np.random.default_rng(seed)
    shape = (height, width)
    count = (rng.integers(1, 9, shape) * 8).astype(np.uint32)
    count[rng.random(shape) < 0.15] = 0
    count[0, 0] = 8  # (an import whose counts are all 0 leaves the accumulator empty, which is a refusal)
    mean = (rng.random(shape + (3,)) * 10.0 ** rng.uniform(-6, 3, shape + (1,))).astype(np.float32)
    total = (mean * count[..., None].astype(np.float32)).astype(np.float32)
    m = np.minimum(rng.integers(0, 9, shape), count >> 3).astype(np.uint32)  # a share with m = 0 or 1: variance unknown
    mom = np.zeros(shape + (4,), np.float32)
    lum = R.lum(mean)
    mom[..., 0] = lum
    mom[..., 1] = (lum * lum * rng.random(shape) * 4.0).astype(np.float32)
    mom[..., 1][rng.random(shape) < 0.1] = 0.0  # zero variance
    mom[..., 2] = m.view(np.float32)
    albedo = rng.random(shape + (3,)).astype(np.float32)
    albedo[rng.random(shape) < 0.1] = 0.0
    # guides that make regions, so that the weights are not all ~0: a few albedos and normals, blockwise, plus jitter
    by, bx = np.meshgrid(np.arange(height) // 7, np.arange(width) // 5, indexing="ij")
    palette = rng.random((8, 3)).astype(np.float32)
    region = (by * 3 + bx) % 8
    albedo = np.where(rng.random(shape)[..., None] < 0.7, palette[region] + rng.normal(0, 0.01, shape + (3,)).astype(np.float32), albedo)
    albedo = np.abs(albedo).astype(np.float32)
    albedo[rng.random(shape) < 0.05] = 0.0
    n = rng.normal(size=(8, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    nn = n[(by + bx) % 8] + rng.normal(0, 0.05, shape + (3,))
    nn *= rng.uniform(0.3, 1.0, shape + (1,)) / np.linalg.norm(nn, axis=-1, keepdims=True)  # averaged guide normals are short, never long
    normal = (0.5 * nn + 0.5).astype(np.float32)
    normal[rng.random(shape) < 0.1] = 0.0  # misses
    state = dict(width=width, height=height, seed=12345, max_depth=14, rr_depth=4, rng=rng.integers(0, 2 ** 32, shape, dtype=np.uint32),
                 sum=total, count=count)
    return state, mom, albedo, normal
