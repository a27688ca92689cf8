"""CPU-side checks (no GPU): the C-ABI library loads and exports every declared symbol, the host-side
scene code (Cornell data, OBJ-free teapot arrays, BVH build, vertex normals, camera) agrees bit for bit
with the oracle and with the golden vectors of the compiled reference, and the device math header
reproduces libm on the arguments the path produces."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import prt_amd
import prt_testlib as T
from prt_images import _jpeg, _png, _png_general, _tga, _write_exr
from prt_testlib import bits


@pytest.fixture(scope="module")
def L():
    prt_amd.build()
    return prt_amd.lib()


def test_library_exports_every_declared_symbol(L):
    declared = set()
    for h in ("prt_hip.h", "prt_host.h"):
        src = open(os.path.join(T.ROOT, "include", h)).read()
        declared |= set(re.findall(r"\b(prt_(?:hip|host)_[a-z0-9_]+)\s*\(", src))
    assert declared == set(prt_amd.EXPORTS), declared ^ set(prt_amd.EXPORTS)
    for name in declared:
        assert hasattr(L, name), name
    # the row-level test entry points live in the TEST build only: the product exports none of them
    src = open(os.path.join(T.ROOT, "include", "prt_hip_test.h")).read()
    rows = set(re.findall(r"\b(prt_hip_[a-z0-9_]+)\s*\(", src))
    assert rows == set(prt_amd.TEST_EXPORTS), rows ^ set(prt_amd.TEST_EXPORTS)
    TL = prt_amd.test_lib()
    for name in rows:
        assert hasattr(TL, name) and not hasattr(L, name), name
    for name in declared:
        assert hasattr(TL, name), name
    syms = subprocess.check_output(["nm", "-D", "--defined-only", prt_amd.LIB_PATH]).decode()
    assert "rays_kernel" not in syms and "leaf_kernel" not in syms and "prt_hip_test" not in syms


def test_rccl_standin_covers_every_symbol_the_product_binds(tmp_path):
    """tests/fake_rccl.cpp (the thread-rank stand-in behind the GPU suite's > 1-rank gather test) must define every ncclXxx the
    product looks up with dlsym (prt_gather.hip), or the product would refuse it on the GPU box; and a PRT_RCCL_LIB that cannot
    be loaded is an error message, never a silent fall-back to another library."""
    src = open(os.path.join(T.ROOT, "prt_amd", "csrc", "prt_gather.hip")).read()
    bound = set(re.findall(r'sym\("(nccl[A-Za-z]+)"\)', src))
    assert len(bound) == 10, bound
    fake = T.build_fake_rccl()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", fake]).decode()
    for name in bound:
        assert f" T {name}" in syms, name
    code = ("import prt_amd, ctypes as C; L = prt_amd.lib(); b = C.create_string_buffer(128); rc = L.prt_hip_comm_unique_id(b); "
            "print(rc, L.prt_hip_last_error().decode())")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PRT_RCCL_LIB=str(tmp_path / "nowhere.so"), PYTHONPATH=T.ROOT),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "PRT_RCCL_LIB=" in out.stdout and not out.stdout.startswith("0 "), out.stdout + out.stderr
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PRT_RCCL_LIB=fake, PYTHONPATH=T.ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("0 "), out.stdout + out.stderr  # the stand-in's ncclGetUniqueId answered


def test_step_loop_has_no_scratch_access():
    """The step loop of the scatter-ray traversal (trace_queue<1, false>: node rounds + cooperative leaf rounds, ~10^9 turns per
    C3 frame) must not touch scratch memory: a spilled value there is a memory round trip per round (round 2's lesson:
    profiles/r02_experiments.txt 6).  tools/step_loop_isa.py compiles the kernel to gfx950 ISA with the product's flags (no GPU
    needed), cuts the loop out by the compiler's loop annotations and lists scratch_ instructions inside it."""
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    import step_loop_isa as S
    lines = S.function_body(S.device_asm())
    loop, body = S.step_loop(lines)
    n, kinds, scratch = S.summary(body)
    assert 300 < n < 2000 and kinds["ds_"] >= 20 and kinds["global_"] >= 10, (n, kinds)  # it IS the step loop
    assert not scratch, "scratch access inside the step loop:\n" + "\n".join(scratch)
    assert kinds["flat_"] == 0 and kinds["buffer_"] == 0, kinds  # global_ / ds_ only: no flat address-space checks
    # the occupancy the design is built around: 64 VGPRs and at most 80 SGPRs (8 waves per SIMD), and two 1024-thread workgroups
    # per CU (their LDS must fit twice into a CU's 160 KB)
    res = S.kernel_resources()
    assert res["VGPRs"] <= 64 and res["TotalSGPRs"] <= 80 and res["Occupancy"] == 8, res
    assert 2 * res["LDS Size"] <= 160 * 1024, res


def test_profile_build_compiles():
    """No product or test build compiles the -DPRT_PROFILE side of prt_stats.h (the real hooks of the trace loops and the host report
    of tools/role_profile.py): this syntax check of the two sources that use it, host and device pass, is its only guard against rot."""
    from prt_amd import _build as B
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC", "-pthread", "-ldl")]
    cmd = [B.hipcc()] + flags + ['-DPRT_SOURCE_SHA16="0"', "-DPRT_PROFILE", "-fsyntax-only"] + [os.path.join(B.CSRC, s) for s in ("prt_kernels.hip", "prt_context.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "error:" not in out.stderr, out.stderr[-4000:]


def test_library_carries_the_hash_of_its_sources(L):
    """prt_amd.build() rebuilds when any kernel source or header is newer than the library (the header list is a glob of csrc/),
    and the library is stamped with the hash of what it was built from: bench.py and the counter summaries quote that stamp."""
    prt_amd.build()
    assert prt_amd.loaded_source_sha16() == prt_amd.source_sha16()
    from prt_amd import _build as B
    assert "prt_frame.h" in B.HEADERS and "prt_device.h" in B.HEADERS


def test_no_gpu_means_loud_failure(L):
    if L.prt_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(prt_amd.PrtError, match="no HIP device"):
        prt_amd.PathTracer()


def test_product_never_links_the_oracle():
    """The oracle is the checker: nothing under prt_amd/ (or the drop-in example) may include, import or link it."""
    out = subprocess.check_output(["ldd", prt_amd.LIB_PATH]).decode()
    assert "oracle" not in out
    pat = re.compile(r"prt_oracle|liboracle|orc_[a-z_]+\(|import\s+prt_testlib|oracle/")
    for top in ("prt_amd", "examples", "include"):
        for root, _, files in os.walk(os.path.join(T.ROOT, top)):
            for f in files:
                if f.endswith((".py", ".cpp", ".h", ".hip", ".inc")):
                    text = open(os.path.join(root, f)).read()
                    assert not pat.search(text), os.path.join(root, f)


def _teapot_mesh():
    m = T.load_teapot_mesh(scale=1.0, translate=(0, 0, 0))
    pm = prt_amd.Mesh.from_arrays(m.indices, m.positions, m.prim_material, m.materials.view(prt_amd.MATERIAL_DTYPE), texcoords=m.texcoords)
    pm.transform(0.005, (-0.5, 0.0, 0.5))
    return pm


def test_cornell_teapot_scene_matches_reference_vectors(L):
    scene, camera, _ = prt_amd.setup_cornell_box(512, 512, teapot_mesh=_teapot_mesh())
    a = scene.arrays()
    z = np.load(os.path.join(T.GOLDEN, "bvh_cornell_teapot.npz"))
    gc = T.load_cornell_mesh()
    assert (a["meshes"][0]["indices"] == gc.indices).all()
    assert (bits(a["meshes"][0]["positions"]) == bits(gc.positions)).all()
    assert a["meshes"][0]["materials"].tobytes() == gc.materials.tobytes()
    assert (bits(a["meshes"][1]["normals"]) == bits(z["teapot_normals"])).all()
    for i in range(2):
        ref = z[f"nodes{i}"].view(T.NODE_DTYPE).reshape(-1)
        got = a["meshes"][i]["nodes"]
        assert len(got) == len(ref)
        for f in ("primOrSecondNodeIndex", "primCount", "splitAxis"):
            assert (got[f] == ref[f]).all(), f
        leaf = ref["primCount"] != 0xF
        assert (got["triVectorIndex"][leaf] == ref["triVectorIndex"][leaf]).all()
        assert (bits(got["lower"]) == bits(ref["lower"])).all() and (bits(got["upper"]) == bits(ref["upper"])).all()
        assert (a["meshes"][i]["remap"] == z[f"remap{i}"]).all()
    assert (bits(scene.bbox()) == bits(z["scene_bbox"])).all()
    assert bits(a["radius"]) == bits(z["radius"])
    cz = np.load(os.path.join(T.GOLDEN, "camera_packets.npz"))["out"][0]
    cam = np.array(list(camera.desc.pos) + list(camera.desc.dir) + list(camera.desc.up) + list(camera.desc.right), dtype=np.float32)
    assert (bits(cam) == bits(cz[96:108])).all()


def test_camera_basis_matches_oracle_for_oblique_views(L):
    for pos, d in (((-15.0, 4.0, 0.5), (1.0, 0.08, -0.05)), ((9, 2.0, 10.2), (0.4, 0.1, -1)), ((0, 5, 0), (0, -1, 0))):
        cam = prt_amd.Camera().create(pos, d, 1920, 1080)
        oc = T.OrcCamera()
        T.oracle().orc_camera_create(C.byref(oc), T.f3(pos), T.f3(d), 1920, 1080)
        for f in ("pos", "dir", "up", "right"):
            assert (bits(np.array(getattr(cam.desc, f)[:], dtype=np.float32)) == bits(np.array(getattr(oc, f)[:], dtype=np.float32))).all(), f
        assert cam.desc.invWidth == oc.invWidth and cam.desc.invHeight == oc.invHeight


def test_obj_reader_matches_teapot_fixture(L, tmp_path):
    import gzip
    path = str(tmp_path / "teapot.obj")  # the reference's data/teapot/teapot.obj, byte for byte (stored gzip-compressed)
    with gzip.open(os.path.join(T.GOLDEN, "teapot.obj.gz"), "rb") as f:
        open(path, "wb").write(f.read())
    scene = prt_amd.Scene()
    m = prt_amd.Mesh.load_obj(path, prt_amd.Material.make(diffuse=(0.9, 0.9, 0.9), reflection=1))
    scene.add(m)
    a = scene.arrays()["meshes"][0]
    z = np.load(os.path.join(T.GOLDEN, "teapot_mesh.npz"))
    assert (a["indices"] == z["indices"]).all()
    assert (bits(a["positions"]) == bits(z["positions"])).all()
    assert (bits(a["texcoords"]) == bits(z["texcoords"])).all()


@pytest.mark.parametrize("n,seed", [(1, 0), (8, 1), (9, 2), (300, 3), (5000, 4)])
def test_bvh_build_matches_oracle_on_random_soups(L, n, seed):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1, 1, (3 * n, 3)).astype(np.float32)
    if seed == 3:
        pos[:, 1] = 0.25  # flat: zero extent on one axis (bvh.cpp:66)
    if seed == 4:
        pos[: 3 * 64] = pos[0]  # many identical centroids: exercises the mid fallback (bvh.cpp:150-153)
    idx = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    nodes_p, cnt, remap_p = C.POINTER(prt_amd.BvhNode)(), C.c_uint32(), C.POINTER(C.c_uint32)()
    assert L.prt_host_bvh_build(n, idx.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), 0, C.byref(nodes_p), C.byref(cnt),
                                C.byref(remap_p)) == 0
    nodes = np.frombuffer(C.string_at(nodes_p, cnt.value * C.sizeof(prt_amd.BvhNode)), dtype=T.NODE_DTYPE).copy()
    remap = np.ctypeslib.as_array(remap_p, shape=(n,)).copy()
    L.prt_host_free(nodes_p)
    L.prt_host_free(remap_p)
    mats = np.array([T.make_material(diffuse=(0.5, 0.5, 0.5))], dtype=T.MATERIAL_DTYPE)
    s = T.OracleScene(T.SceneDesc([T.MeshDesc(idx, pos, np.zeros(n, dtype=np.uint32), mats)], (0, 0, 3), (0, 0, -1), 8, 8))
    on = s.nodes(0)
    assert len(on) == len(nodes)
    assert on.tobytes() == nodes.tobytes()
    assert (s.prim_remap(0) == remap).all()


def test_devmath_matches_libm_on_every_path_argument(tmp_path):
    """sincos: all 2^23 theta = 2*pi*r1 the bounce can produce, every float in [-0.5, 10] and a 1/61 sample of the whole float line
    (environment light angles: both reductions of glibc's sinf / cosf, below and from 120, infinities, NaN);
    powf(x, 2.2): every float in [2^-24, 2] and a 1/13 sample below (a bilinear texel mix can leave [0, 1] by a rounding)."""
    src = tmp_path / "dm.c"
    src.write_text(r'''
#include <stdio.h>
#include <math.h>
#include <string.h>
#include "%s/prt_amd/csrc/prt_devmath.h"
int main(){ const float kPi = 3.14159265358979323846f; long bad=0;
  for(uint32_t k=0;k<(1u<<23);k++){ uint32_t b=k|0x3f800000u; float f; memcpy(&f,&b,4); float theta=2.0f*kPi*(f-1.0f);
    float s,c; prt_sincosf(theta,&s,&c); float gs=sinf(theta), gc=cosf(theta);
    if(memcmp(&s,&gs,4)||memcmp(&c,&gc,4)) bad++; }
  /* environment light (light.cpp:121-125): theta = 2*pi*(u+0.5), phi = pi*v with u, v a little below 0 up to 1: every float in [-0.5, 0) and [0, 10] */
  for(int neg=0;neg<2;neg++){ float top=neg?0.5f:10.0f; uint32_t hi; memcpy(&hi,&top,4);
    for(uint32_t b=0;b<=hi;b++){ uint32_t bb=b|(neg?0x80000000u:0u); float y; memcpy(&y,&bb,4);
      float s,c; prt_sincosf(y,&s,&c); float gs=sinf(y), gc=cosf(y); if(memcmp(&s,&gs,4)||memcmp(&c,&gc,4)) bad++; } }
  /* ... and a bright texel in the first row or column of the environment map makes (u, v) any size and sign: every 61st bit pattern of the
     whole float line (all 2^32 were checked once: 0 mismatches), infinities and NaNs included */
  for(uint64_t b=0;b<(1ull<<32);b+=61){ uint32_t bb=(uint32_t)b; float y; memcpy(&y,&bb,4);
    float s,c; prt_sincosf(y,&s,&c); float gs=sinf(y), gc=cosf(y);
    if(!((isnan(gs)? isnan(s) : !memcmp(&s,&gs,4)) && (isnan(gc)? isnan(c) : !memcmp(&c,&gc,4)))) bad++; }
  for(uint32_t b=0x33800000u;b<=0x3f800000u;b++){ float x; memcpy(&x,&b,4); float m=prt_powf_2p2(x), g=powf(x,2.2f); if(memcmp(&m,&g,4)) bad++; }
  float z=0.0f, m=prt_powf_2p2(z), g=powf(z,2.2f); if(memcmp(&m,&g,4)) bad++;
  /* a bilinear mix can leave [2^-24, 1] by a rounding (weights that sum to 1 + ulp; a weight of 1e-8): every float in [1, 2] and every 13th
     below 2^-24, denormals included (all of [0, 2] were checked once: 0 mismatches) */
  for(uint32_t b=0x3f800000u;b<=0x40000000u;b++){ float x; memcpy(&x,&b,4); float mm=prt_powf_2p2(x), gg=powf(x,2.2f); if(memcmp(&mm,&gg,4)) bad++; }
  for(uint32_t b=0;b<0x33800000u;b+=13){ float x; memcpy(&x,&b,4); float mm=prt_powf_2p2(x), gg=powf(x,2.2f); if(memcmp(&mm,&gg,4)) bad++; }
  printf("%%ld\n", bad); return 0; }
''' % T.ROOT)
    exe = tmp_path / "dm"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", str(src), "-o", str(exe), "-lm"])
    assert subprocess.check_output([str(exe)]).decode().strip() == "0"


def test_infinite_area_light_tables_match_oracle(L, tmp_path):
    """Scene::setInfiniteAreaLight -> InfiniteAreaLight::create (light.cpp:30-84) on the host: the CDF tables handed to the
    kernels equal the oracle's (which equal the compiled reference's, tests/golden/env_light.npz), from memory and from a PFM."""
    env = T.sky_env(48, 24, black_rows=True)
    scene, camera, exposure = prt_amd.setup_cornell_box(64, 64)
    scene.set_infinite_area_light(env)
    a = scene.arrays()
    desc = T.scene_desc_from_product(scene, camera, exposure)
    s = T.OracleScene(desc)
    vp, hp = s.env_tables()
    assert np.array_equal(a["env"].view(np.uint32), env.view(np.uint32))
    assert np.array_equal(a["env_vertical"].view(np.uint32), vp.view(np.uint32))
    assert np.array_equal(a["env_horizontal"].view(np.uint32), hp.view(np.uint32))
    z = np.load(os.path.join(T.GOLDEN, "env_light.npz"))
    assert np.array_equal(a["env_vertical"].view(np.uint32), z["black_rows_vertical"].view(np.uint32))
    # the same map through a little-endian PFM (rows bottom to top)
    p = tmp_path / "env.pfm"
    with open(p, "wb") as f:
        f.write(b"PF\n48 24\n-1.0\n")
        f.write(np.ascontiguousarray(env[::-1, :, :3], dtype="<f4").tobytes())
    scene2, _, _ = prt_amd.setup_cornell_box(64, 64)
    scene2.set_infinite_area_light(str(p))
    b = scene2.arrays()
    assert np.array_equal(b["env"].view(np.uint32), env.view(np.uint32))
    assert np.array_equal(b["env_horizontal"].view(np.uint32), hp.view(np.uint32))
    scene3, _, _ = prt_amd.setup_cornell_box(64, 64)
    with pytest.raises(prt_amd.PrtError):
        scene3.set_infinite_area_light(str(tmp_path / "missing.pfm"))
    assert scene3.arrays()["env"] is None


def test_environment_map_from_openexr(L, tmp_path):
    """Scene::setInfiniteAreaLight(path) decodes an OpenEXR file in the reference (texture.cpp:256-310: tinyexr LoadEXR -> RGBA
    float32, top row first).  tinyexr is absent; the reader here takes scan-line files with NO / RLE / ZIPS / ZIP blocks and UINT /
    HALF / FLOAT channels: the product's own writer's files (HALF B, G, R: ZIP and raw), a test-side writer's files with float
    channels incl. alpha, a data window off the origin, smooth rows (so that RLE runs and ZIP both bite) and a grey file; the CDF
    tables built from the decoded texels equal those of the same texels passed in memory; PIZ is refused."""
    rng = np.random.default_rng(11)
    h, w = 37, 50  # three ZIP blocks, the last one short
    rgb = (rng.random((h, w, 3), dtype=np.float32) * 6.0).astype(np.float32)
    rgb[5:9] = 0.25  # constant rows
    for zipped in (True, False):
        p = tmp_path / f"own_{int(zipped)}.exr"
        prt_amd.save_exr(str(p), rgb, zip=zipped)
        scene, _, _ = prt_amd.setup_cornell_box(32, 32)
        scene.set_infinite_area_light(str(p))
        got = scene.arrays()
        want = np.concatenate([rgb.astype(np.float16).astype(np.float32), np.ones((h, w, 1), np.float32)], axis=2)
        assert np.array_equal(got["env"].view(np.uint32), want.view(np.uint32)), f"own writer, zip={zipped}"
        ref, _, _ = prt_amd.setup_cornell_box(32, 32)
        ref.set_infinite_area_light(want)
        assert np.array_equal(ref.arrays()["env_horizontal"].view(np.uint32), got["env_horizontal"].view(np.uint32))
        assert np.array_equal(ref.arrays()["env_vertical"].view(np.uint32), got["env_vertical"].view(np.uint32))
    smooth = np.linspace(0.0, 4.0, w, dtype=np.float32)[None, :].repeat(h, 0)
    chans = {"R": rgb[..., 0].copy(), "G": smooth.copy(), "B": rgb[..., 2].astype(np.float16), "A": np.full((h, w), 0.5, np.float32),
             "Z": rng.integers(0, 1000, (h, w)).astype(np.uint32)}  # Z: an extra channel the reader has to step over
    for comp in (0, 1, 2, 3):
        p = tmp_path / f"t{comp}.exr"
        _write_exr(str(p), chans, 3, 5, comp)
        scene, _, _ = prt_amd.setup_cornell_box(32, 32)
        scene.set_infinite_area_light(str(p))
        got = scene.arrays()["env"]
        want = np.stack([chans["R"], chans["G"], chans["B"].astype(np.float32), chans["A"]], axis=2)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"compression {comp}"
    _write_exr(str(tmp_path / "grey.exr"), {"Y": rgb[..., 1].astype(np.float16)}, 0, 0, 3)
    scene, _, _ = prt_amd.setup_cornell_box(32, 32)
    scene.set_infinite_area_light(str(tmp_path / "grey.exr"))
    g = rgb[..., 1].astype(np.float16).astype(np.float32)
    assert np.array_equal(scene.arrays()["env"], np.stack([g, g, g, np.ones_like(g)], axis=2))
    _write_exr(str(tmp_path / "piz.exr"), {"R": rgb[..., 0]}, 0, 0, 0)
    raw = bytearray(open(tmp_path / "piz.exr", "rb").read())
    i = raw.index(b"compression\0compression\0") + len(b"compression\0compression\0") + 4
    raw[i] = 4  # PIZ
    open(tmp_path / "piz.exr", "wb").write(raw)
    scene, _, _ = prt_amd.setup_cornell_box(32, 32)
    with pytest.raises(prt_amd.PrtError):
        scene.set_infinite_area_light(str(tmp_path / "piz.exr"))
    assert scene.arrays()["env"] is None
    # a crafted file must be refused, not crash the host: block offsets near 2^64 (where `off + 8` wraps), beyond the file, and a
    # channel list cut off in the middle of an entry
    import struct
    _write_exr(str(tmp_path / "ok.exr"), {"R": rgb[..., 0]}, 0, 0, 0)
    good = bytearray(open(tmp_path / "ok.exr", "rb").read())
    # the offset table follows the header's terminating NUL: find it as the first 8-byte value that points inside the file at a block whose y is 0
    table = next(k for k in range(8, len(good) - 16) if 0 < struct.unpack_from("<Q", good, k)[0] < len(good) - 8
                 and struct.unpack_from("<i", good, struct.unpack_from("<Q", good, k)[0])[0] == 0 and good[k - 1] == 0)
    for bad in (0xFFFFFFFFFFFFFFFC, 0xFFFFFFFFFFFFFFF8, len(good) - 4, len(good) + 1000):
        raw = bytearray(good)
        struct.pack_into("<Q", raw, table, bad)
        open(tmp_path / "bad.exr", "wb").write(raw)
        scene, _, _ = prt_amd.setup_cornell_box(32, 32)
        with pytest.raises(prt_amd.PrtError):
            scene.set_infinite_area_light(str(tmp_path / "bad.exr"))
    cut = good.index(b"channels\0chlist\0") + len(b"channels\0chlist\0") + 4 + 2 + 4 + 2  # inside the first entry: name "R\0", type, 2 of the 4 pLinear bytes
    open(tmp_path / "cut.exr", "wb").write(bytes(good[:cut]))
    scene, _, _ = prt_amd.setup_cornell_box(32, 32)
    with pytest.raises(prt_amd.PrtError):
        scene.set_infinite_area_light(str(tmp_path / "cut.exr"))


@pytest.mark.parametrize("rle", [False, True])
@pytest.mark.parametrize("top_down", [False, True])
def test_obj_mtl_reader_decodes_tga_maps(L, tmp_path, rle, top_down):
    """map_Kd / map_bump through TGA files (true-colour with alpha, grey; raw and run-length encoded; both row orders):
    texels reach the scene descriptor as Texture::load would deliver them (RGBA for colour, one component for grey,
    texture.cpp:226-247), and the alpha channel switches the alpha test on (material.cpp:79)."""
    rng = np.random.default_rng(3)
    kd = rng.integers(0, 256, size=(6, 9, 4), dtype=np.uint8)
    kd[2:4, :, :] = kd[2, 0]            # runs for the RLE path
    kd[..., 3] = np.where(rng.random((6, 9)) < 0.5, 255, 40)
    bump = rng.integers(0, 256, size=(5, 7), dtype=np.uint8)
    bump[1] = 77
    _tga(tmp_path / "kd.tga", kd, rle, top_down)
    _tga(tmp_path / "bump.tga", bump, rle, top_down)
    (tmp_path / "m.mtl").write_text("newmtl a\nKd 1 1 1\nmap_Kd kd.tga\nmap_bump -bm 1.0 bump.tga\n")
    (tmp_path / "m.obj").write_text("mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl a\nf 1/1 2/2 3/3\n")
    scene = prt_amd.Scene()
    scene.add(prt_amd.Mesh.load_obj(str(tmp_path / "m.obj")))
    a = scene.arrays()
    mats = a["meshes"][0]["materials"]
    assert len(a["textures"]) == 2 and int(mats["alphaTest"][0]) == 1
    assert np.array_equal(a["textures"][int(mats["diffuseMap"][0])], kd)
    assert np.array_equal(a["textures"][int(mats["bumpMap"][0])][..., 0], bump)


@pytest.mark.parametrize("level,strategy", [(0, 0), (1, 0), (9, 0), (6, 4)])  # stored, dynamic Huffman, fixed Huffman (Z_FIXED)
def test_obj_mtl_reader_decodes_png_maps(L, tmp_path, level, strategy):
    rng = np.random.default_rng(5)
    kd = rng.integers(0, 256, size=(13, 11, 4), dtype=np.uint8)
    kd[3:9, 2:9] = kd[3, 2]  # long matches for the LZ77 path
    kd[..., 3] = np.where(rng.random((13, 11)) < 0.5, 255, 17)
    grey = (np.arange(19 * 7, dtype=np.uint32).reshape(7, 19) * 7 % 256).astype(np.uint8)
    _png(tmp_path / "kd.png", kd, level, strategy)
    _png(tmp_path / "bump.png", grey, level, strategy)
    (tmp_path / "m.mtl").write_text("newmtl a\nKd 1 1 1\nmap_Kd kd.png\nmap_bump bump.png\n")
    (tmp_path / "m.obj").write_text("mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl a\nf 1/1 2/2 3/3\n")
    scene = prt_amd.Scene()
    scene.add(prt_amd.Mesh.load_obj(str(tmp_path / "m.obj")))
    a = scene.arrays()
    mats = a["meshes"][0]["materials"]
    assert np.array_equal(a["textures"][int(mats["diffuseMap"][0])], kd) and int(mats["alphaTest"][0]) == 1
    assert np.array_equal(a["textures"][int(mats["bumpMap"][0])][..., 0], grey)
    # RGB (no alpha -> 255, no alpha test), grey + alpha, and a palette with transparency
    rgb = rng.integers(0, 256, size=(5, 6, 3), dtype=np.uint8)
    ga = rng.integers(0, 256, size=(4, 5, 2), dtype=np.uint8)
    pal = rng.integers(0, 256, size=(7, 3), dtype=np.uint8)
    idx = rng.integers(0, 7, size=(6, 4), dtype=np.uint8)
    tr = np.array([255, 0, 128], dtype=np.uint8)
    _png(tmp_path / "rgb.png", rgb, level, strategy)
    _png(tmp_path / "ga.png", ga, level, strategy)
    _png(tmp_path / "pal.png", idx, level, strategy, palette=pal, trns=tr)
    for name, want in (("rgb", np.dstack([rgb, np.full(rgb.shape[:2], 255, np.uint8)])),
                       ("ga", np.dstack([ga[..., 0], ga[..., 0], ga[..., 0], ga[..., 1]])),
                       ("pal", np.dstack([pal[idx], np.where(idx < 3, tr[np.minimum(idx, 2)], 255).astype(np.uint8)]))):
        (tmp_path / "n.mtl").write_text(f"newmtl a\nKd 1 1 1\nmap_Kd {name}.png\n")
        (tmp_path / "n.obj").write_text("mtllib n.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl a\nf 1/1 2/2 3/3\n")
        sc = prt_amd.Scene()
        sc.add(prt_amd.Mesh.load_obj(str(tmp_path / "n.obj")))
        b = sc.arrays()
        assert np.array_equal(b["textures"][0], want), name


@pytest.mark.parametrize("interlace", [False, True])
def test_png_bit_depths_interlace_and_colour_keys(L, tmp_path, interlace):
    """The PNG files stb_image accepts beyond plain 8-bit ones (texture.cpp:218-249 asks it for 8 bits per channel): 16-bit
    samples keep their high byte, 1 / 2 / 4-bit grey is scaled to 0..255, palettes of 1 / 2 / 4 bits, Adam7 interlace, and a
    colour key (tRNS) adds an alpha channel that is 0 exactly where the pixel equals the key."""
    import struct
    rng = np.random.default_rng(11)
    h, w = 11, 13  # not multiples of 8: every Adam7 pass has a ragged edge

    def load(name):
        (tmp_path / "n.mtl").write_text(f"newmtl a\nKd 1 1 1\nmap_Kd {name}\n")
        (tmp_path / "n.obj").write_text("mtllib n.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl a\nf 1/1 2/2 3/3\n")
        sc = prt_amd.Scene()
        sc.add(prt_amd.Mesh.load_obj(str(tmp_path / "n.obj")))
        return sc.arrays()["textures"][0]

    def rgba(x):  # what Texture::load keeps (texture.cpp:218-249): one channel for a grey file, else RGBA (alpha 255 if the file has none)
        if x.shape[2] == 1: pass
        elif x.shape[2] == 2: x = np.dstack([x[..., 0], x[..., 0], x[..., 0], x[..., 1]])
        elif x.shape[2] == 3: x = np.dstack([x, np.full(x.shape[:2], 255)])
        return x.astype(np.uint8)

    for ch, ctype in ((1, 0), (2, 4), (3, 2), (4, 6)):  # 16 bits per sample
        v = rng.integers(0, 65536, size=(h, w, ch))
        _png_general(tmp_path / "a.png", v, 16, ctype, interlace)
        assert np.array_equal(load("a.png"), rgba(v >> 8)), (ch, "16-bit")
    for bits, scale in ((1, 255), (2, 85), (4, 17)):  # grey below 8 bits, and palettes
        v = rng.integers(0, 1 << bits, size=(h, w, 1))
        _png_general(tmp_path / "g.png", v, bits, 0, interlace)
        assert np.array_equal(load("g.png"), rgba(v * scale)), (bits, "grey")
        pal = rng.integers(0, 256, size=(1 << bits, 3))
        _png_general(tmp_path / "p.png", v, bits, 3, interlace, palette=pal)
        assert np.array_equal(load("p.png"), rgba(pal[v[..., 0]])), (bits, "palette")
    # colour keys: 8-bit RGB, 16-bit grey
    v = rng.integers(0, 256, size=(h, w, 3))
    v[2:5, 3:6] = (10, 200, 30)
    _png_general(tmp_path / "k.png", v, 8, 2, interlace, trns=struct.pack(">HHH", 10, 200, 30))
    want = np.dstack([v, np.where((v == (10, 200, 30)).all(-1), 0, 255)]).astype(np.uint8)
    assert np.array_equal(load("k.png"), want)
    g = rng.integers(0, 65536, size=(h, w, 1))
    g[1, 1] = g[7, 9] = 0x1234
    _png_general(tmp_path / "k16.png", g, 16, 0, interlace, trns=struct.pack(">H", 0x1234))
    want = np.dstack([g[..., 0] >> 8] * 3 + [np.where(g[..., 0] == 0x1234, 0, 255)]).astype(np.uint8)
    assert np.array_equal(load("k16.png"), want)


def _load_texture_through_obj(tmp_path, name):
    (tmp_path / "q.mtl").write_text(f"newmtl a\nKd 1 1 1\nmap_Kd {name}\n")
    (tmp_path / "q.obj").write_text("mtllib q.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl a\nf 1/1 2/2 3/3\n")
    sc = prt_amd.Scene()
    sc.add(prt_amd.Mesh.load_obj(str(tmp_path / "q.obj")))
    return sc.arrays()["textures"][0]


def test_png_and_jpeg_files_written_by_an_independent_library(L, tmp_path):
    """The texture decoders against files they did not write themselves: Pillow (libpng / libjpeg) encodes, where it is
    installed, and the decoders must give libpng's pixels exactly and libjpeg's within the arithmetic difference between two
    conforming JPEG decoders (stb_image's integer IDCT and fixed-point YCbCr, which the decoder restates, against libjpeg's).
    Covers what the test-side writers cannot vouch for: real Huffman and quantisation tables, optimised tables, restart
    intervals, 4:4:4 / 4:2:2 / 4:2:0 sampling, progressive files, palette files with transparency, zlib streams of several block types."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    h, w = 61, 83  # ragged against 8 and 16
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(xx * 3) % 256, (yy * 4) % 256, ((xx + yy) * 2) % 256], axis=2).astype(np.uint8)
    noisy = np.clip(smooth.astype(np.int32) + rng.integers(-20, 21, smooth.shape), 0, 255).astype(np.uint8)

    def expect(im):  # Texture::load (texture.cpp:218-249): one channel for grey files, RGBA otherwise
        a = np.asarray(im)
        if a.ndim == 2: return a[..., None]
        if a.shape[2] == 2: return np.dstack([a[..., 0]] * 3 + [a[..., 1]])
        if a.shape[2] == 3: return np.dstack([a, np.full(a.shape[:2], 255, np.uint8)])
        return a

    # ---- PNG: exact
    for mode, arr in (("RGB", noisy), ("RGBA", np.dstack([noisy, smooth[..., 0]])), ("L", noisy[..., 0]), ("LA", np.dstack([noisy[..., 0], smooth[..., 1]]))):
        for level in (0, 1, 9):
            Image.fromarray(arr, mode).save(tmp_path / "a.png", compress_level=level)
            assert np.array_equal(_load_texture_through_obj(tmp_path, "a.png"), expect(Image.open(tmp_path / "a.png"))), (mode, level)
    pal = Image.fromarray(noisy, "RGB").quantize(37)
    pal.save(tmp_path / "p.png", transparency=5)
    got = _load_texture_through_obj(tmp_path, "p.png")
    assert np.array_equal(got, np.asarray(Image.open(tmp_path / "p.png").convert("RGBA"))), "palette with transparency"
    # interlaced and 16-bit files from the test-side writer: Pillow must read them as the decoder does (the writer is sound too)
    v8 = rng.integers(0, 256, size=(h, w, 4))
    _png_general(tmp_path / "i.png", v8, 8, 6, True)
    assert np.array_equal(_load_texture_through_obj(tmp_path, "i.png"), np.asarray(Image.open(tmp_path / "i.png").convert("RGBA"))), "Adam7"
    assert np.array_equal(np.asarray(Image.open(tmp_path / "i.png")), v8.astype(np.uint8))
    # ---- TGA: exact (24 / 32 bit, raw and run-length encoded)
    for mode, arr in (("RGB", noisy), ("RGBA", np.dstack([smooth, noisy[..., 2]])), ("L", smooth[..., 0])):
        for comp in (None, "tga_rle"):
            Image.fromarray(arr, mode).save(tmp_path / "a.tga", **({"compression": comp} if comp else {}))
            assert np.array_equal(_load_texture_through_obj(tmp_path, "a.tga"), expect(Image.open(tmp_path / "a.tga"))), (mode, comp)
    # ---- JPEG: within the difference between two conforming decoders
    for name, kw, tol in (("444 q95", dict(quality=95, subsampling=0), 3), ("422 q90", dict(quality=90, subsampling=1), 6),
                          ("420 q85 optimised", dict(quality=85, subsampling=2, optimize=True), 8), ("420 q60", dict(quality=60, subsampling=2), 8)):
        Image.fromarray(smooth, "RGB").save(tmp_path / "a.jpg", **kw)
        got = _load_texture_through_obj(tmp_path, "a.jpg").astype(np.int32)
        want = expect(Image.open(tmp_path / "a.jpg").convert("RGB")).astype(np.int32)
        assert got.shape == want.shape, name
        d = np.abs(got - want)
        if kw["subsampling"] == 1:
            # stb_image's horizontal 2x resampler weighs the last pair of a row the other way round than libjpeg
            # ((3 * in[w-2] + in[w-1]) / 4 where libjpeg has 3 * in[w-1] + in[w-2]); the decoder follows stb_image, so the last
            # two columns are compared loosely
            assert d[:, -2:].max() <= 128
            d = d[:, :-2]
        assert d.max() <= tol and d.mean() < 0.8, (name, int(d.max()), float(d.mean()))
    Image.fromarray(noisy[..., 0], "L").save(tmp_path / "g.jpg", quality=92)
    got = _load_texture_through_obj(tmp_path, "g.jpg").astype(np.int32)
    want = expect(Image.open(tmp_path / "g.jpg")).astype(np.int32)
    assert got.shape == want.shape and np.abs(got - want).max() <= 2, "grey"
    # progressive files (SOF2: spectral selection and successive approximation, DC and AC refinement scans, end-of-band runs)
    for name, arr, mode, kw, tol in (("progressive 444", smooth, "RGB", dict(quality=92, subsampling=0), 3), ("progressive 420", smooth, "RGB", dict(quality=80, subsampling=2), 8),
                                     ("progressive 420 noisy", noisy, "RGB", dict(quality=50, subsampling=2), 10), ("progressive grey", noisy[..., 1], "L", dict(quality=88), 2)):
        Image.fromarray(arr, mode).save(tmp_path / "pr.jpg", progressive=True, **kw)
        assert b"\xff\xc2" in open(tmp_path / "pr.jpg", "rb").read(), "the file is not progressive"
        got = _load_texture_through_obj(tmp_path, "pr.jpg").astype(np.int32)
        want = expect(Image.open(tmp_path / "pr.jpg").convert(mode)).astype(np.int32)
        assert got.shape == want.shape, name
        d = np.abs(got - want)
        assert d.max() <= tol and d.mean() < 0.9, (name, int(d.max()), float(d.mean()))
    raw = bytearray(open(tmp_path / "pr.jpg", "rb").read())
    raw[raw.index(b"\xff\xc2") + 1] = 0xc9  # arithmetic coding: refused with a message (the material keeps no map), not misread
    open(tmp_path / "ar.jpg", "wb").write(raw)
    with pytest.raises(IndexError):
        _load_texture_through_obj(tmp_path, "ar.jpg")


@pytest.mark.parametrize("sampling,restart", [([(1, 1)], 0), ([(1, 1), (1, 1), (1, 1)], 0), ([(2, 2), (1, 1), (1, 1)], 3), ([(2, 1), (1, 1), (1, 1)], 0),
                                              ([(1, 2), (1, 1), (1, 1)], 5)])
def test_obj_mtl_reader_decodes_jpeg_maps(L, tmp_path, sampling, restart):
    """Sequential JPEG textures (the format of Sponza's and San Miguel's maps; texture.cpp:218-249 reads them through
    stb_image): grey and YCbCr files with 4:4:4, 4:2:0, 4:2:2 and 4:4:0 sampling and restart intervals come back within the
    quantisation and chroma-filter error of the image that was encoded, grey as one channel, colour as RGBA with alpha 255."""
    rng = np.random.default_rng(21)
    H, W = 37, 45  # ragged against every MCU size
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = lambda a, b, c: (127 + 90 * np.sin(xx / a + c) * np.cos(yy / b)).clip(0, 255)  # noqa: E731
    Y = smooth(7.0, 5.0, 0.3)
    Y[10:20, 12:30] = 230  # an edge
    planes = [Y] if len(sampling) == 1 else [Y, smooth(15.0, 11.0, 1.0), smooth(13.0, 17.0, 2.0)]
    planes = [np.round(p).astype(np.uint8) for p in planes]
    _jpeg(tmp_path / "t.jpg", planes, sampling, q=2, restart=restart)
    (tmp_path / "n.mtl").write_text("newmtl a\nKd 1 1 1\nmap_Kd t.jpg\n")
    (tmp_path / "n.obj").write_text("mtllib n.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl a\nf 1/1 2/2 3/3\n")
    sc = prt_amd.Scene()
    sc.add(prt_amd.Mesh.load_obj(str(tmp_path / "n.obj")))
    tex = sc.arrays()["textures"][0].astype(np.int32)
    if len(sampling) == 1:
        assert tex.shape == (H, W, 1)
        assert np.abs(tex[..., 0] - planes[0]).max() <= 4
        return
    assert tex.shape == (H, W, 4) and (tex[..., 3] == 255).all()
    y, cb, cr = (p.astype(np.float64) for p in planes)
    want = np.stack([y + 1.402 * (cr - 128), y - 0.344136 * (cb - 128) - 0.714136 * (cr - 128), y + 1.772 * (cb - 128)], -1).clip(0, 255)
    err = np.abs(tex[..., :3] - want)
    sub = sampling[0] != (1, 1)
    assert err.mean() < (2.5 if sub else 1.5) and np.percentile(err, 99) <= (12 if sub else 6), (err.mean(), err.max())


def _read_exr_halfs(raw, w, h):
    """Parse a scan-line OpenEXR file with three HALF channels B, G, R (NO or ZIP compression): (h, 3, w) uint16 and the attributes."""
    import struct
    import zlib
    assert struct.unpack_from("<ii", raw, 0) == (20000630, 2)
    o, attrs = 8, {}
    while raw[o] != 0:
        e = raw.index(b"\0", o); name = raw[o:e].decode(); o = e + 1
        e = raw.index(b"\0", o); typ = raw[o:e].decode(); o = e + 1
        (size,) = struct.unpack_from("<i", raw, o); o += 4
        attrs[name] = (typ, raw[o:o + size]); o += size
    o += 1
    comp = attrs["compression"][1][0]
    lines = {0: 1, 3: 16}[comp]
    blocks = (h + lines - 1) // lines
    offs = struct.unpack_from(f"<{blocks}Q", raw, o)
    out = np.zeros((h, 3, w), dtype=np.uint16)
    for b in range(blocks):
        yy, size = struct.unpack_from("<ii", raw, offs[b])
        assert yy == b * lines
        n_lines = min(lines, h - yy)
        want = n_lines * w * 3 * 2
        data = raw[offs[b] + 8: offs[b] + 8 + size]
        if comp == 3 and size < want:
            t = np.frombuffer(zlib.decompress(data), dtype=np.uint8).astype(np.int32)  # a real zlib stream
            assert len(t) == want
            t = (np.cumsum(np.concatenate([t[:1], t[1:] - 128])) & 255).astype(np.uint8)  # undo the delta predictor
            half = (want + 1) // 2
            data = np.empty(want, dtype=np.uint8)
            data[0::2], data[1::2] = t[:half], t[half:]  # undo the even / odd byte split
            data = data.tobytes()
        assert len(data) == want
        out[yy:yy + n_lines] = np.frombuffer(data, dtype="<u2").reshape(n_lines, 3, w)
    return out, attrs


def test_exr_and_ppm_writers(L, tmp_path):
    """Image::saveExr (image.cpp:82-139): half-float B, G, R planes in a scan-line OpenEXR -- ZIP-compressed blocks of 16 lines
    (tinyexr's default in the reference) or raw lines; parsed back (the ZIP blocks through Python's zlib), every sample must
    be the round-to-nearest-even half of the float.  Image::savePpm (image.cpp:52-80)."""
    import struct
    rng = np.random.default_rng(9)
    h, w = 37, 13  # three blocks of 16 lines, the last one short
    img = (rng.random((h, w, 3), dtype=np.float32) * np.float32(4.0)).astype(np.float32)
    img[8:30] = np.float32(0.5)  # smooth rows: blocks that really shrink
    specials = np.array([0.0, -0.0, 1e-8, 5.96e-8, 2.98e-8, 2.9802322e-8, 6.1e-5, 6.0975552e-5, 65504.0, 65519.9, 65520.0, 1e9, np.inf, -np.inf,
                         np.nan, 1.0009765625, 1.00048828125, 1.00146484375, 0.33333334, -2.5, 1023.75, 2047.5, 2048.5], dtype=np.float32)
    img.reshape(-1)[:len(specials)] = specials
    with np.errstate(over="ignore"):
        want = img.astype(np.float16)
    sizes = {}
    for zip_ in (True, False):
        p = tmp_path / "o.exr"
        prt_amd.save_exr(str(p), img, zip=zip_)
        raw = open(p, "rb").read()
        sizes[zip_] = len(raw)
        halfs, attrs = _read_exr_halfs(raw, w, h)
        assert attrs["compression"] == ("compression", b"\3" if zip_ else b"\0") and attrs["lineOrder"][1] == b"\0"
        assert struct.unpack("<4i", attrs["dataWindow"][1]) == (0, 0, w - 1, h - 1)
        ch = attrs["channels"][1]
        assert [ch[i * 18:i * 18 + 1] for i in range(3)] == [b"B", b"G", b"R"] and struct.unpack_from("<i", ch, 2)[0] == 1  # HALF
        for y in range(h):
            for k, c in enumerate((2, 1, 0)):  # B, G, R
                got, exp = halfs[y, k], want[y, :, c].view(np.uint16)
                nan = np.isnan(want[y, :, c])
                assert np.array_equal(got[~nan], exp[~nan]), (y, c)
                assert ((got[nan] & 0x7c00) == 0x7c00).all() and ((got[nan] & 0x3ff) != 0).all()
    assert sizes[True] < 0.8 * sizes[False]
    # PPM: c/(c+1), clamp, pow(1/2.2), * 255, truncate
    q = tmp_path / "o.ppm"
    fin = np.nan_to_num(img, nan=0.0, posinf=1e30, neginf=0.0)
    prt_amd.save_ppm(str(q), fin, tonemap=True)
    data = open(q, "rb").read()
    assert data.startswith(b"P6\n%d %d\n255\n" % (w, h))
    px = np.frombuffer(data[-w * h * 3:], dtype=np.uint8).reshape(h, w, 3)
    c = fin.astype(np.float64)
    ref = np.clip(c / (c + 1.0), 0.0, 1.0) ** (1.0 / 2.2) * 255.0
    assert (np.abs(px.astype(np.float64) - np.floor(ref)) <= 1).all()


@pytest.mark.ref
def test_reference_main_cpp_compiles_and_links_unmodified(L):
    """The drop-in claim of SURVEY.md 8b, checked on the reference's own caller: its src/main.cpp, byte for byte, is compiled
    against include/prt_compat/ (one forwarding header per reference header it includes, each pulling in
    prt_amd/csrc/host/prt.h) and linked against libprt_hip.so -- with and without PRT_ENABLE_STATS (main.cpp:148-152,
    176-178).  oracle/Makefile does it where the reference's tree is present (oracle/_ref/prt_ref_main{,_stats}, reached
    through a link so that its `#include "scene.h"` resolves to the compat directory, not to the reference's headers beside it);
    here, every header it depended on must be the project's and the library must provide what it calls.  (Running it needs
    an MI355X and the reference's teapot asset: examples/main.cpp is the stand-in that the GPU tests run.)"""
    for name in ("prt_ref_main", "prt_ref_main_stats"):
        exe = os.path.join(T.REF_DIR, name)
        if not os.path.exists(exe):
            pytest.skip(f"oracle/_ref/{name} is only built where the reference's tree is present")
        deps = open(exe + ".d").read().replace("\\\n", " ").split(":", 1)[1].split()
        assert deps[0] == "_ref/main.cpp"
        for d in deps[1:]:  # (-MMD: system headers are not listed)
            assert os.path.realpath(os.path.join(T.ORACLE_DIR, d)).startswith(T.ROOT + os.sep), f"{name} compiled against {d}"
        assert any(d.endswith("prt_compat/scene.h") for d in deps) and any(d.endswith("host/prt.h") for d in deps)
        syms = subprocess.check_output(["nm", "-u", "-C", exe]).decode()
        for needed in ("prt::PathTracer::TraceBlock", "prt::Bvh::build", "prt::Scene::add", "prt::Image::saveExr", "prt::ThreadPool::queue"):
            assert needed in syms, needed


def test_bench_roofline_binds_on_a_measured_roof_of_the_committed_counters():
    """bench.py's `roofline.frac` is the LARGEST of three measured roofs (useful vector-ALU share, L2-miss rate against the measured gather
    ceiling of the tree's size, HBM bytes), each <= 1, from the committed counter summary of the workload -- never the algorithmic figure,
    which exceeds 1 on the headline configuration.  The summaries under profiles/ must carry the stamp of the kernel
    sources in the tree: bench.py ignores a stale one and would then report `frac: null` to the driver."""
    import importlib.util
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    expect = {"c3": ("valu_useful", 13.3e6), "c4": ("l2_miss_rate", 127.7e6), "c5share": ("l2_miss_rate", 255e6)}
    for w, (bound, tree) in expect.items():
        ev = json.load(open(os.path.join(root, "profiles", f"r04_frame_{w}_counters.json")))
        assert ev["source_sha16"] == prt_amd.source_sha16(), f"profiles/r04_frame_{w}_counters.json was taken with other kernel sources: collect it again (tools/collect_counters.sh)"
        name, roofs = bench.binding_roof(ev, ev["kernel_ms_under_profiler_median"], tree)
        assert name == bound, (w, name)
        assert all(0.0 < r["frac"] <= 1.0 for r in roofs.values()), (w, {k: r["frac"] for k, r in roofs.items()})
        assert roofs[name]["frac"] == max(r["frac"] for r in roofs.values())
    # the table of gather ceilings is monotone in the table size
    sizes = [g for _, g, _ in bench.GATHER_ROOF]
    assert sizes == sorted(sizes, reverse=True)
