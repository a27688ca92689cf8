"""Radiance queries on the MI355X (include/prt_hip.h "radiance"; the CPU half is tests/test_probe_cpu.py): prt_hip_query_radiance of the
PRODUCT library against the live oracle -- probe q is pixel (0, 0) of orc_trace_block under the degenerate camera at rays[q] with seed
seed + q (tests/prt_probe_ref.py) -- and against the product's own camera path.  Everything at tolerance 0."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import prt_amd
import prt_hostile_shade as HS
import prt_probe_ref as PR
import prt_testlib as T
from prt_gpukit import SCENES

pytestmark = pytest.mark.gpu
F = np.float32
DEPTH = 8
POOL_GROUPS = 16 * 64   # PRT_POOL_CHUNKS rows of PRT_CHUNK pixel groups per workgroup (prt_frame.h)
BLOCKS_PER_CU = 2       # a workgroup of the frame kernel holds 78 576 B of the CU's 160 KB of LDS
UNWRITTEN = 0xffc0bad1  # a NaN no probe produces: the scenes here hold no NaN, and arithmetic gives the default NaN


class Case:
    def __init__(self, name):
        self.scene, self.camera = SCENES[name]()
        self.desc = T.scene_desc_from_product(self.scene, self.camera, 1.0)
        self.oracle = T.OracleScene(self.desc)
        self.t = prt_amd.PathTracer(max_depth=DEPTH)
        self.t.upload_scene(self.scene)  # no camera is set: a radiance query needs none


@pytest.fixture(scope="module")
def cases():
    prt_amd.build()
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name)
        return made[name]
    yield get
    for c in made.values():
        c.t.close()


def same_rows(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} probes differ, first {bad[:4]}: {got[bad[0]]} != {want[bad[0]]}")


def raw_query(t, rays, out, spp, seed, depth=DEPTH, flags=prt_amd.QUERY_HOST, n=None, stream=None, **fields):
    """prt_hip_query_radiance itself: returns the code; fields override render parameters."""
    p = t.params(spp, max_depth=depth)
    p.seed = seed
    for k, v in fields.items():
        setattr(p, k, v)
    rp = rays if isinstance(rays, int) else rays.ctypes.data_as(C.c_void_p)
    op = out if isinstance(out, int) else out.ctypes.data_as(C.c_void_p)
    return t._L.prt_hip_query_radiance(t._ctx, len(rays) if n is None else n, rp, C.byref(p), op, flags, stream)


# ----------------------------------------------------------------------------- 1. the oracle
@pytest.fixture(scope="module")
def stage_answers(cases):
    """Per scene the 1000 probes of test 1 and the oracle's radiance for spp 8 and 24, computed once."""
    out = {}
    for name in ("plain", "sky"):
        org, d = PR.stage_probes(1000, seed=11)
        out[name] = dict(org=org, dir=d, seed=31337)
    return out


@pytest.mark.parametrize("spp", [8, 24])
@pytest.mark.parametrize("n", [1, 7, 64, 65, 1000])
@pytest.mark.parametrize("name", ["plain", "sky"])
def test_probes_equal_the_oracle(cases, stage_answers, name, n, spp):
    c, a = cases(name), stage_answers[name]
    org, d, seed = a["org"][:n], a["dir"][:n], a["seed"]
    key = ("want", spp)
    if key not in a:  # the prefix of the full batch is the full batch's prefix: probe q depends on q alone
        a[key] = PR.trace(c.oracle, a["org"], a["dir"], spp, DEPTH, seed)[0]
    _, rays, occl = PR.trace(c.oracle, org, d, spp, DEPTH, seed)
    got = c.t.query_radiance(org, d, spp, seed=seed)
    assert got.shape == (n, 3) and got.dtype == F
    same_rows(got, a[key][:n], f"{name}, {n} probes at {spp} spp")
    st = c.t.last_stats
    assert (st["raysTraced"], st["occludedTraced"], st["nPx"]) == (rays, occl, n), (st, rays, occl)
    assert st["kernelLaunches"] == 1 and st["kernelMs"] > 0 and st["stackOverflow"] == 0
    if n >= 64:
        lit = int((got != 0).any(axis=1).sum())
        print(f"{name} n={n} spp={spp}: {lit} probes are not black")
        assert lit > n // 4


# ----------------------------------------------------------------------------- 2. the product's own camera path
def test_probes_equal_one_pixel_renders_under_the_degenerate_camera(cases, stage_answers):
    """The header's definition, independently of the oracle: set_camera with pos = org, dir = dir, up = right = 0, 1 x 1; render with
    seed + q; download."""
    c, a = cases("plain"), stage_answers["plain"]
    org, d, seed, spp = a["org"][:32], a["dir"][:32], 977, 16
    got = c.t.query_radiance(org, d, spp, seed=seed, exposure=1.25)
    other = prt_amd.PathTracer(max_depth=DEPTH)
    try:
        other.upload_scene(c.scene)
        for q in range(32):
            other.seed = (seed + q) & 0xffffffff
            other.set_camera(PR.product_camera(org[q], d[q]))
            px = other.render(spp, exposure=1.25)
            assert px.shape == (1, 1, 3)
            assert px.reshape(3).tobytes() == got[q].tobytes(), (q, px, got[q])
    finally:
        other.close()
    assert (got != 0).any(axis=1).sum() > 8


# ----------------------------------------------------------------------------- 3. indices beyond 16 bits
def test_probe_indices_are_not_split_into_16_bit_halves(cases):
    c = cases("plain")
    n, spp, depth, seed = 65536 + 130, 8, 4, 2024
    org, d = PR.stage_probes(n, seed=13)
    org[65536:], d[65536:] = org[:130], d[:130]  # probe q + 65536 is probe q's ray under another seed
    want, rays, occl = PR.trace(c.oracle, org, d, spp, depth, seed)
    got = c.t.query_radiance(org, d, spp, seed=seed, max_depth=depth)
    same_rows(got, want, "65666 probes")
    st = c.t.last_stats
    assert (st["raysTraced"], st["occludedTraced"], st["nPx"]) == (rays, occl, n)
    # probe q and probe q + 65536 share a ray and differ by their seeds -- wherever the estimate draws a number at all: a probe that
    # sees the sunlit floor and whose bounces all leave the open stage is the direct light alone, under any seed (the oracle's pairs
    # say which; a kernel that dropped the high half of the index would make EVERY pair equal)
    differ = (got[:130].view(np.uint32) != got[65536:].view(np.uint32)).any(axis=1)
    assert (differ == (want[:130].view(np.uint32) != want[65536:].view(np.uint32)).any(axis=1)).all()
    print("pairs (q, q + 65536) that differ:", int(differ.sum()), "of 130")
    assert differ.sum() >= 30, "probe q and probe q + 65536 must differ by their seeds"


# ----------------------------------------------------------------------------- 4. beyond the pool
def test_a_batch_larger_than_the_pool_recycles_rows_and_ends_ragged(cases):
    c = cases("plain")
    capacity = c.t.device_info()[1] * BLOCKS_PER_CU * POOL_GROUPS
    n, spp, depth, seed = capacity + 64 * 3 + 5, 8, 2, 555
    assert n % 64 != 0 and n <= 1 << 24
    base_org, base_d = PR.stage_probes(4099, seed=17)  # (a prime: the tiling does not line up with rows or blocks)
    idx = np.arange(n) % 4099
    org, d = base_org[idx], base_d[idx]
    rays = prt_amd.make_rays(org, d, 0.0)
    out = np.full((n, 3), UNWRITTEN, dtype=np.uint32).view(F)
    assert raw_query(c.t, rays, out, spp, seed, depth=depth) == 0, c.t._L.prt_hip_last_error()
    st = c.t.stats()
    assert st["nPx"] == n and st["kernelLaunches"] == 1 and st["stackOverflow"] == 0
    assert not (out.view(np.uint32) == UNWRITTEN).any(), "probes the launch never wrote"
    which = np.unique(np.concatenate([np.arange(128), np.arange(n - 128, n), np.arange(128, n - 128, 251)]))
    assert len(which) >= 2000
    want, _, _ = PR.trace(c.oracle, org, d, spp, depth, seed, which=which)
    same_rows(out[which], want[which], f"{len(which)} of {n} probes")
    assert (out[which] != 0).any(axis=1).sum() > len(which) // 4


# ----------------------------------------------------------------------------- 5. hostile probes
@pytest.mark.parametrize("name", ["plain", "box_rr"])
def test_hostile_probes_equal_the_oracle_and_leave_their_neighbours_alone(cases, name):
    c = cases(name)
    org, d, at = PR.hostile_case(name)
    spp, seed = 16, 4242
    want, rays, occl = PR.trace(c.oracle, org, d, spp, DEPTH, seed)
    got = c.t.query_radiance(org, d, spp, seed=seed)
    same_rows(got, want, f"{name}: the batch with the hostile probes")  # (bytes: a NaN would have to carry the oracle's payload)
    st = c.t.last_stats
    assert (st["raysTraced"], st["occludedTraced"], st["nPx"]) == (rays, occl, 64)
    for k in [PR.HOSTILE.index(h) for h in PR.DEGENERATE + ("nan_org",)]:
        assert got[at[k]].tobytes() == np.zeros(3, F).tobytes(), PR.HOSTILE[k]
    # the same batch with ordinary probes in the hostile places: the others keep their answers (their seeds go by index)
    tame_org, tame_d = org.copy(), d.copy()
    tame_org[at], tame_d[at] = org[at - 1], d[at - 1]
    tame = c.t.query_radiance(tame_org, tame_d, spp, seed=seed)
    rest = np.ones(64, bool)
    rest[at] = False
    same_rows(tame[rest], got[rest], f"{name}: the ordinary probes without the hostile ones")
    assert (got[rest] != 0).any(axis=1).sum() > rest.sum() // 4


# ----------------------------------------------------------------------------- 6. side effects
def test_a_radiance_query_leaves_the_context_alone(cases):
    c = cases("plain")
    t = prt_amd.PathTracer(max_depth=DEPTH)
    try:
        t.upload_scene(c.scene)
        t.set_camera(c.camera)
        want16 = t.render(16)
        t.accumulate(8)
        t.denoise_temporal(iterations=2)
        t.set_camera(c.camera)  # the pending record becomes the history; the accumulator is emptied
        t.adaptive_pass(8, 0.05, 8, 64)  # (an adaptive pass: the moments hold something)
        t.denoise_temporal(iterations=2)
        t.display(prt_amd.DisplayParams.make(meter=True))
        W, H = c.camera.width, c.camera.height

        def snapshot():
            acc = t.accum_export()
            hist, pend = t.history_export(0), t.history_export(1)
            return dict(rng=acc["rng"], sum=acc["sum"], count=acc["count"], bound=np.array([acc["seed"], acc["max_depth"], acc["rr_depth"]]),
                        moments=t.accum_export_moments(), **{f"hist_{k}": hist[k] for k in ("color_var", "pos_len", "normal")},
                        **{f"pend_{k}": pend[k] for k in ("color_var", "pos_len", "normal")},
                        display=np.frombuffer(repr(sorted(t.display_state().items())).encode(), np.uint8),
                        framebuffer=t._download_rect(0, 0, W - 1, H - 1, stats=False))
        before = snapshot()
        assert before["count"].any() and before["moments"].any() and before["framebuffer"].any()
        t.stats()
        org, d = PR.stage_probes(300, seed=19)
        got = t.query_radiance(org, d, 8, seed=5)
        same_rows(got, PR.trace(c.oracle, org, d, 8, DEPTH, 5)[0], "the query between the passes")
        assert t.last_stats["kernelLaunches"] == 1 and t.last_stats["nPx"] == 300
        after = snapshot()
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k
        assert t.accumulate(8).tobytes() == want16.tobytes(), "the accumulate pass behind the query continues the one-shot render"
    finally:
        t.close()


# ----------------------------------------------------------------------------- 7. device pointers and streams
def test_device_tensors_on_a_callers_stream():
    """tests/probe_torch_stream.py in a process of its own (torch must load its HIP runtime before the library binds to one): torch
    tensors on a non-default stream, the query behind a kernel that writes the rays and in front of one that reads the radiance,
    equal to the host path (which test 1 holds to the oracle on this scene)."""
    prt_amd.build()
    r = subprocess.run([sys.executable, os.path.join(T.ROOT, "tests", "probe_torch_stream.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok 3000 probes" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ----------------------------------------------------------------------------- 8. scene edits
def test_probes_follow_mesh_updates_and_light_edits():
    prt_amd.build()
    scene, camera = HS.scene("plain")
    t = prt_amd.PathTracer(max_depth=DEPTH)
    try:
        t.upload_scene(scene)
        org, d = PR.stage_probes(500, seed=29)
        spp, seed = 8, 66
        first = t.query_radiance(org, d, spp, seed=seed)
        same_rows(first, PR.trace(T.OracleScene(T.scene_desc_from_product(scene, camera, 1.0)), org, d, spp, DEPTH, seed)[0], "before the edits")
        a = scene.arrays()["meshes"]
        moved = (a[0]["positions"] + np.array([0.4, 0.0, 0.3], F)).astype(F)
        scene.update_positions(0, moved)
        t.update_meshes(scene, [0])
        second = t.query_radiance(org, d, spp, seed=seed)
        same_rows(second, PR.trace(T.OracleScene(T.scene_desc_from_product(scene, camera, 1.0)), org, d, spp, DEPTH, seed)[0], "after update_meshes")
        assert second.tobytes() != first.tobytes()
        scene.set_directional_light((-0.5, 0.8, 0.2), (1.0, 4.0, 2.0))
        t.update_lights(scene)
        third = t.query_radiance(org, d, spp, seed=seed)
        same_rows(third, PR.trace(T.OracleScene(T.scene_desc_from_product(scene, camera, 1.0)), org, d, spp, DEPTH, seed)[0], "after update_lights")
        assert third.tobytes() != second.tobytes()
    finally:
        t.close()


# ----------------------------------------------------------------------------- 9. refusals
def test_refusals_launch_nothing_and_a_camera_is_not_needed():
    prt_amd.build()
    scene, _ = HS.scene("plain")
    t = prt_amd.PathTracer(max_depth=DEPTH)
    try:
        L = t._L
        org, d = PR.stage_probes(16, seed=37)
        rays = prt_amd.make_rays(org, d, 0.0)
        out = np.full((16, 3), UNWRITTEN, dtype=np.uint32).view(F)
        assert raw_query(t, rays, out, 8, 1) == -5 and b"upload a scene" in L.prt_hip_last_error()
        t.upload_scene(scene)  # no camera is ever set
        t.stats()
        bad = [dict(spp=0), dict(spp=12), dict(spp=2048), dict(nranks=2), dict(rank=1, nranks=2), dict(countTraffic=1), dict(n=0), dict(n=(1 << 24) + 1),
               dict(flags=prt_amd.QUERY_HOST | 2), dict(flags=0x80000000)]
        for kw in bad:
            kw = dict(kw)
            rc = raw_query(t, rays, out, kw.pop("spp", 8), 1, n=kw.pop("n", None), flags=kw.pop("flags", prt_amd.QUERY_HOST), **kw)
            assert rc == -2 and L.prt_hip_last_error(), (kw, rc, L.prt_hip_last_error())
        with prt_amd.DeviceArrays() as dev:
            dptr = dev.alloc(4096)
            assert raw_query(t, dptr + 8, dptr + 2048, 8, 1, flags=0, n=16) == -2 and b"16-byte aligned" in L.prt_hip_last_error()
            assert raw_query(t, dptr, dptr + 2050, 8, 1, flags=0, n=16) == -2 and b"4-byte aligned" in L.prt_hip_last_error()
        assert t.stats()["kernelLaunches"] == 0
        assert (out.view(np.uint32) == UNWRITTEN).all(), "a refused call wrote radiance"
        assert raw_query(t, rays, out, 8, 1) == 0, L.prt_hip_last_error()  # success without a camera
        same_rows(out, PR.trace(T.OracleScene(T.scene_desc_from_product(scene, HS.scene("plain")[1], 1.0)), org, d, 8, DEPTH, 1)[0], "without a camera")
        assert t.stats()["nPx"] == 16
    finally:
        t.close()
