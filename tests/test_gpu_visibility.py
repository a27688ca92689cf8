"""Visibility baking on the MI355X (include/prt_hip.h "visibility baking"; the CPU half is tests/test_visibility_cpu.py):
prt_hip_bake_visibility of the PRODUCT library against its definition, composed by the test from calls that are pinned elsewhere --
the bytes against prt_hip_query_any of the rays of prt_hip_bake_rays with tMax set, the sums against the numpy restatement
tests/prt_visibility_ref.py of those bytes.  Everything at tolerance 0, compared as bytes, with sentinels behind every output.  The
scenes, points and direction sets are tests/prt_visibility_cases.py: chosen so that a constant answer cannot pass."""
import ctypes as C

import numpy as np
import pytest

import prt_amd
import prt_bake_ref as BR
import prt_hostile_shade as HS
import prt_probe_ref as PR
import prt_testlib as T
import prt_visibility_cases as VC
import prt_visibility_ref as VR
from prt_gpukit import SENTINEL, TAIL, fetch, ptr, sentinel, stage_tracers
from prt_gpukit import dev  # noqa: F401  (fixture: device memory and streams for one test)

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
HOST = prt_amd.QUERY_HOST
INF = float("inf")
BYTE = 0xa5      # what an occlusion array holds before a call: neither answer
BYTE_TAIL = 64   # sentinel bytes behind every occlusion array


def teapot_scene():  # (the teapot stage of tests/test_gpu_atlas.py)
    return prt_amd.setup_cornell_box(8, 8, teapot_mesh=T.teapot_product_mesh())[0]


tracers = stage_tracers(dict(VC.SCENES, teapot=teapot_scene), arrays=True, max_depth=8)  # tracers(name) -> (context, mesh arrays)


def table(sets, dirs="host", weights="host", **fields):
    """prt_bake_sets of `sets`; dirs / weights: "host", None (a NULL pointer) or a device address (int)."""
    t = prt_amd.BakeSets(K=sets.K, C=sets.C, nSets=sets.nSets, reserved=0, dirs=sets.dirs.ctypes.data if dirs == "host" else dirs,
                         weights=sets.weights.ctypes.data if weights == "host" else weights)
    for k, v in fields.items():
        setattr(t, k, v)
    return t


def vis_params(md=INF, triple=False, flags=None, reserved=(0, 0)):
    v = prt_amd.VisibilityParams(md, (prt_amd.VIS_TRIPLE if triple else 0) if flags is None else flags)
    v.reserved[0], v.reserved[1] = reserved
    return v


def byte_sentinel(n):
    return np.full(n + BYTE_TAIL, BYTE, np.uint8)


def run(t, dev, pts, sets, md=INF, triple=False, want_bytes=True, device=False, stream=None):
    """prt_hip_bake_visibility on host or device arrays: (out words followed by sentinel words, bytes followed by sentinel bytes or None)."""
    n, rep = len(pts), 3 if triple else 1
    out, occ = sentinel(n * sets.C * rep + TAIL), byte_sentinel(n * sets.K) if want_bytes else None
    v = vis_params(md, triple)
    if not device:
        tb = table(sets)
        rc = t._L.prt_hip_bake_visibility(t._ctx, n, ptr(pts), C.byref(tb), C.byref(v), ptr(out), ptr(occ), HOST, None)
        assert rc == 0, t._L.prt_hip_last_error()
        return out, occ
    d_pts, d_dirs, d_w, d_out = (dev.upload(a) for a in (pts, sets.dirs, sets.weights, out))
    d_occ = dev.upload(occ) if want_bytes else None
    tb = table(sets, dirs=d_dirs, weights=d_w)
    rc = t._L.prt_hip_bake_visibility(t._ctx, n, d_pts, C.byref(tb), C.byref(v), d_out, d_occ, 0, stream)
    assert rc == 0, t._L.prt_hip_last_error()
    return fetch(dev, d_out, out.size), fetch(dev, d_occ, occ.size, np.uint8) if want_bytes else None


def composed_bytes(t, pts, sets, md):
    """prt_hip_query_any of the rays of prt_hip_bake_rays with tMax = md: (n * K,) uint8."""
    r = t.bake_rays(pts["P"], pts["N"], sets.dirs, bias=pts["bias"], sets=pts["set"])
    return t.query_any(r["org"], r["dir"], md)


def check(got, want_occ, pts, sets, triple, what):
    """The product's (out, bytes) against the expected bytes and the restatement of their sums; the sentinels behind both."""
    out, occ = got
    want = VR.reduce(pts, sets, want_occ, triple)
    if occ is not None:
        assert occ[:len(want_occ)].tobytes() == want_occ.tobytes(), f"{what}: {int((occ[:len(want_occ)] != want_occ).sum())} of {len(want_occ)} bytes differ"
        assert (occ[len(want_occ):] == BYTE).all(), f"{what}: bytes behind the occlusion array were written"
    BR.same_bytes(out[:want.size], want, what)
    assert (out[want.size:] == SENTINEL).all(), f"{what}: words behind out were written"
    return want


def shares(occ):
    ones = float((occ != 0).mean())
    return min(ones, 1.0 - ones)


# ----------------------------------------------------------------------------- 1. fused equals composed
@pytest.mark.parametrize("Cc", [1, 3, 9])
@pytest.mark.parametrize("nSets", [1, 3])
@pytest.mark.parametrize("K", [1, 7, 64, 65, 300])
@pytest.mark.parametrize("name", ["plain", "box_rr", "atrium"])
def test_fused_equals_composed(tracers, dev, name, K, nSets, Cc):
    t, _ = tracers(name)
    pts, sets = VC.make_points(name, nSets), VC.make_sets(nSets, K, Cc)
    want = {md: composed_bytes(t, pts, sets, md) for md in (INF, VC.finite_distance(name))}
    # the condition, on the expected bytes: a constant answer cannot pass, and the finite distance opens rays that +inf closes
    far, near = want[INF], want[VC.finite_distance(name)]
    print(f"{name} K={K} nSets={nSets}: occluded {far.mean():.3f} under +inf, {near.mean():.3f} under {VC.finite_distance(name):.3f}")
    assert shares(far) >= 0.1 and shares(near) >= 0.1 and ((far == 1) & (near == 0)).any()
    assert set(np.unique(far)) == {0, 1} and not far.reshape(len(pts), K)[[30, 33]].any(), "a set outside the table"
    for md, occ in want.items():
        for triple in (False, True):
            check(run(t, dev, pts, sets, md, triple), occ, pts, sets, triple, f"{name} K={K} nSets={nSets} C={Cc} maxDistance={md} triple={triple}")
    # without the caller's array the bytes stay in the context and the sums are the same; device pointers give the same bytes
    check(run(t, dev, pts, sets, INF, want_bytes=False), far, pts, sets, False, "no byte array")
    check(run(t, dev, pts, sets, VC.finite_distance(name), triple=True, device=True), near, pts, sets, True, "device pointers")
    if K == 65 and Cc == 3:  # the Python wrappers are the same calls
        out, occ = t.bake_visibility(pts["P"], pts["N"], sets.dirs, sets.weights, bias=pts["bias"], sets=pts["set"], return_bytes=True)
        assert out.shape == (len(pts), Cc) and occ.shape == (len(pts), K) and occ.reshape(-1).tobytes() == far.tobytes()
        BR.same_bytes(out, VR.reduce(pts, sets, far), "bake_visibility()")
        again = t.bake_visibility_reduce(sets.weights, occ, sets=pts["set"], triple=True)
        BR.same_bytes(again, VR.reduce(pts, sets, far, triple=True), "bake_visibility_reduce()")


# ----------------------------------------------------------------------------- 2. beyond one claim of the cursor
def test_more_rays_than_the_static_ranges_with_waves_that_straddle_points(tracers, dev):
    """trace_loop (prt_device.h) gives every wave a static range of `chunk` rays and hands out what lies beyond waves * chunk through
    the claim cursor, chunk = n / (4 * waves) held to 64 .. 1024.  The launch is two workgroups of 16 waves per compute unit
    (PRT_VIS_TRACE_BLOCKS_PER_CU, prt_visibility.hip): on 256 compute units 8192 waves, chunk = 64 at this size, so the static ranges
    end at ray 524 288 -- which is also the number of lanes launched -- and the other half of the rays is claimed.  K = 37 divides
    neither 64 nor the chunk: nearly every wave straddles two or three points."""
    t, _ = tracers("plain")
    K, nSets = 37, 3
    n = ((1 << 20) + K - 1) // K + 3
    waves = t.device_info()[1] * 2 * 16
    chunk = min(max(n * K // (4 * waves), 64), 1024)
    assert n * K > waves * chunk + 64 * chunk, "rays beyond the static ranges, more than one claim of them"
    base = VC.make_points("plain", nSets)
    pts = np.tile(base, n // len(base) + 1)[:n].copy()
    rng = np.random.default_rng(21)
    pts["P"] += rng.uniform(-0.03, 0.03, (n, 3)).astype(F)  # (no two points alike)
    sets = VC.make_sets(nSets, K, 1)
    want = composed_bytes(t, pts, sets, INF)
    print(f"{n} points x {K} directions = {n * K} rays, {waves} waves x chunk {chunk}: occluded {want.mean():.3f}")
    assert shares(want) >= 0.1
    check(run(t, dev, pts, sets, INF), want, pts, sets, False, f"{n * K} rays")
    st = t.stats()
    assert st["raysTraced"] == st["occludedTraced"] == n * K and st["stackOverflow"] == 0


# ----------------------------------------------------------------------------- 3. the reduce half alone
def run_reduce(t, dev, pts, sets, occ, triple, device):
    n, rep = len(pts), 3 if triple else 1
    out = sentinel(n * sets.C * rep + TAIL)
    v = vis_params(INF, triple)
    if not device:
        tb = table(sets, dirs=None)
        rc = t._L.prt_hip_bake_visibility_reduce(t._ctx, n, ptr(pts), C.byref(tb), C.byref(v), ptr(occ), ptr(out), HOST, None)
        assert rc == 0, t._L.prt_hip_last_error()
        return out
    d_pts, d_w, d_occ, d_out = (dev.upload(a) for a in (pts, sets.weights, occ, out))
    tb = table(sets, dirs=None, weights=d_w)
    rc = t._L.prt_hip_bake_visibility_reduce(t._ctx, n, d_pts, C.byref(tb), C.byref(v), d_occ, d_out, 0, None)
    assert rc == 0, t._L.prt_hip_last_error()
    return fetch(dev, d_out, out.size)


@pytest.mark.parametrize("K,Cc", [(4096, 3), (257, 2), (256, 16), (65, 9), (1, 1)])
def test_the_reduce_half_on_synthetic_bytes(tracers, dev, K, Cc):
    """Needs no scene.  Bytes other than 0 and 1 (any non-zero byte is occluded), -0.0 and NaN weights, sets outside the table; K on
    both sides of the 256 directions a lane keeps in a register."""
    t, _ = tracers("none")
    n, nSets = 37, 2
    rng = np.random.default_rng(K)
    w = (rng.uniform(0.0, 1.0, (nSets, K, Cc)) * 10.0 ** rng.uniform(-3, 3, (nSets, K, Cc))).astype(F)
    w[rng.random(w.shape) < 0.05] = -0.0
    w[1, K // 2, Cc - 1] = np.nan
    sets = BR.Sets(np.zeros((nSets, K, 3), F), w)
    occ = rng.choice(np.array([0, 0, 0, 1, 2, 128, 255], np.uint8), size=(n, K))
    s = (np.arange(n) % nSets).astype(U)
    s[30], s[33] = nSets, 0xffffffff
    occ[1, K // 2], occ[3, K // 2], occ[5], occ[6], occ[7] = 0, 200, 0, 1, 255  # point 1 sees the NaN weight, point 3 does not
    pts = BR.points(np.zeros((n, 3)), np.zeros((n, 3)), 0.0, s)
    for triple in (False, True):
        want = VR.reduce(pts, sets, occ, triple)
        nan = np.isnan(want.reshape(n, Cc, -1)[:, :, 0])
        assert nan[1, Cc - 1] and not nan[3].any() and nan.sum() == sum(1 for i in range(1, n, 2) if occ[i, K // 2] == 0 and s[i] == 1)
        assert not want[[6, 7, 30, 33]].view(U).any(), "+0 for a closed point and for a set outside the table"
        host = run_reduce(t, dev, pts, sets, occ.reshape(-1), triple, device=False)
        BR.same_bytes(host[:want.size], want, f"K={K} C={Cc} triple={triple}, host arrays")
        assert (host[want.size:] == SENTINEL).all(), "words behind out were written"
        assert run_reduce(t, dev, pts, sets, occ.reshape(-1), triple, device=True).tobytes() == host.tobytes(), "device and host pointers differ"


# ----------------------------------------------------------------------------- 4. hostile points
def test_hostile_points_equal_the_composition_and_leave_their_neighbours_alone(tracers, dev):
    t, _ = tracers("plain")
    K, nSets = 65, 3
    calm, sets = VC.make_points("plain", nSets), VC.make_sets(nSets, K, 3)
    nan = np.array([PR.NAN_PAYLOAD], dtype=U).view(F)[0]
    pts = calm.copy()
    hostile = {8: ("N", (nan, 1.0, 0.0)), 9: ("N", (0.0, np.inf, 0.0)), 10: ("N", (1e-30, 1e-30, 0.0)), 11: ("N", (0.0, 3e20, 1e20)),
               12: ("P", (0.0, nan, 0.0)), 13: ("bias", nan), 14: ("N", (-np.inf, 1.0, nan))}
    for i, (field, value) in hostile.items():
        pts[field][i] = value
    t.stats()
    for md in (INF, VC.finite_distance("plain")):
        want = composed_bytes(t, pts, sets, md)
        got = run(t, dev, pts, sets, md)
        check(got, want, pts, sets, False, f"hostile points, maxDistance={md}")
        assert not want.reshape(-1, K)[[8, 9, 12, 13, 14]].any(), "a ray with a NaN in it is not occluded"
        base = run(t, dev, calm, sets, md)
        keep = np.array([i not in hostile for i in range(len(pts))])
        assert got[1][:len(want)].reshape(-1, K)[keep].tobytes() == base[1][:len(want)].reshape(-1, K)[keep].tobytes()
        assert got[0][:len(pts) * 3].reshape(-1, 3)[keep].tobytes() == base[0][:len(pts) * 3].reshape(-1, 3)[keep].tobytes()
    assert t.stats()["stackOverflow"] == 0


# ----------------------------------------------------------------------------- 5. analytic, tolerance 0
def test_a_point_outside_sees_everything_and_a_point_under_the_ceiling_nothing(tracers, dev):
    """VC.closed_case says why its rays stay in a cone: which faces of box_rr an any-hit ray can end on is prt_hip_query_any's rule."""
    t, _ = tracers("plain")
    pts, sets = VC.open_case()
    out, occ = run(t, dev, pts, sets)
    assert not occ[:len(pts) * 64].any() and out[:len(pts)].tobytes() == np.ones(len(pts), F).tobytes(), "exactly 1.0f"
    t, _ = tracers("box_rr")
    pts, sets = VC.closed_case()
    out, occ = run(t, dev, pts, sets)
    assert (occ[:len(pts) * 64] == 1).all() and not out[:len(pts) * 2].any(), "+0"
    out, _ = run(t, dev, pts, sets, triple=True)
    assert not out[:len(pts) * 6].any() and (out[len(pts) * 6:] == SENTINEL).all()


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals_queue_nothing_and_leave_the_outputs_untouched(tracers, dev):
    (t, _), (bare, _) = tracers("plain"), tracers("none")
    L = t._L
    pts, sets = VC.make_points("plain", 3), VC.make_sets(3, 8, 2)
    n = len(pts)
    out, occ, occ_in = sentinel(n * 2 * 3 + TAIL), byte_sentinel(n * 8), np.zeros(n * 8, np.uint8)

    def both(ctx, n_=n, p=ptr(pts), tb=None, v=None, o=ptr(out), flags=HOST, b=ptr(occ), b_in=ptr(occ_in)):
        tb = table(sets) if tb is None else tb
        v = vis_params() if v is None else v
        tbp, vp = (None if tb == "null" else C.byref(tb)), (None if v == "null" else C.byref(v))
        return (L.prt_hip_bake_visibility(ctx, n_, p, tbp, vp, o, b, flags, None), L.prt_hip_bake_visibility_reduce(ctx, n_, p, tbp, vp, b_in, o, flags, None))
    t.stats()
    # without a scene: the trace half only
    trace, reduce_ = both(bare._ctx)
    assert trace == -5 and reduce_ == 0
    assert L.prt_hip_bake_visibility(bare._ctx, n, ptr(pts), C.byref(table(sets)), C.byref(vis_params()), ptr(out), None, HOST, None) == -5
    assert b"upload a scene" in L.prt_hip_last_error()
    out[:] = SENTINEL  # (the reduce half on the bare context was accepted)
    big = prt_amd.BakeSets(K=4096, C=1, nSets=1, reserved=0, dirs=sets.dirs.ctypes.data, weights=sets.weights.ctypes.data)
    cases = [dict(tb=table(sets, **kw)) for kw in (dict(K=0), dict(K=4097), dict(C=0), dict(C=17), dict(nSets=0), dict(nSets=1025), dict(reserved=1))]
    cases += [dict(n_=0), dict(tb=big, n_=(1 << 18) + 1), dict(flags=HOST | 2), dict(flags=0x80000000)]
    cases += [dict(v=vis_params(md)) for md in (np.nan, 0.0, -0.0, -1.0, -np.inf)]
    cases += [dict(v=vis_params(flags=2)), dict(v=vis_params(flags=0x80000001)), dict(v=vis_params(reserved=(1, 0))), dict(v=vis_params(reserved=(0, 7)))]
    cases += [dict(p=None), dict(tb="null"), dict(v="null"), dict(o=None), dict(tb=table(sets, weights=None))]
    for kw in cases:
        assert both(t._ctx, **kw) == (-2, -2) and L.prt_hip_last_error(), kw
    assert L.prt_hip_bake_visibility(t._ctx, n, ptr(pts), C.byref(table(sets, dirs=None)), C.byref(vis_params()), ptr(out), ptr(occ), HOST, None) == -2
    assert L.prt_hip_bake_visibility_reduce(t._ctx, n, ptr(pts), C.byref(table(sets)), C.byref(vis_params()), None, ptr(out), HOST, None) == -2
    # device pointers that are not aligned
    base = dev.upload(np.zeros(1 << 16, np.uint8))
    dt, v = table(sets, dirs=base, weights=base + 4096), vis_params()
    for args in ((base + 8192 + 8, dt, base + 16384), (base + 8192, dt, base + 16384 + 2), (base + 8192, table(sets, dirs=base + 2, weights=base + 4096), base + 16384)):
        assert L.prt_hip_bake_visibility(t._ctx, n, args[0], C.byref(args[1]), C.byref(v), args[2], base + 32768, 0, None) == -2
        assert b"aligned" in L.prt_hip_last_error()
    assert L.prt_hip_bake_visibility_reduce(t._ctx, n, base + 8192, C.byref(table(sets, dirs=None, weights=base + 4096 + 1)), C.byref(v), base + 32768, base + 16384, 0, None) == -2
    assert not fetch(dev, base, 1 << 16, np.uint8).any(), "a refused call wrote device memory"
    assert t.stats()["kernelLaunches"] == 0
    assert (out == SENTINEL).all() and (occ == BYTE).all(), "a refused call wrote its output"
    assert both(t._ctx) == (0, 0) and not (out[:n * 2] == SENTINEL).any()  # and the same arguments are accepted
    assert both(t._ctx, tb=table(sets, dirs=None), b=None) == (-2, 0)      # the reduce half reads no directions,
    assert L.prt_hip_bake_visibility(t._ctx, n, ptr(pts), C.byref(table(sets)), C.byref(vis_params()), ptr(out), None, HOST, None) == 0  # the trace half needs no byte array


# ----------------------------------------------------------------------------- 7. state and statistics
def test_a_visibility_bake_leaves_the_context_alone(dev):
    prt_amd.build()
    scene, camera = HS.scene("plain")
    t = prt_amd.PathTracer(max_depth=8)
    try:
        t.upload_scene(scene)
        t.set_camera(camera)
        want16 = t.render(16)
        t.accumulate(8)
        t.display(prt_amd.DisplayParams.make(meter=True))
        W, H = camera.width, camera.height
        org, d = PR.stage_probes(100, seed=23)
        probes = t.query_radiance(org, d, 8, seed=5)  # (the staging arena holds this batch)

        def snapshot():
            acc = t.accum_export()
            return dict(rng=acc["rng"], sum=acc["sum"], count=acc["count"], bound=np.array([acc["seed"], acc["max_depth"], acc["rr_depth"]]),
                        display=np.frombuffer(repr(sorted(t.display_state().items())).encode(), np.uint8),
                        framebuffer=t._download_rect(0, 0, W - 1, H - 1, stats=False))
        pts, sets = VC.make_points("plain", 3), VC.make_sets(3, 65, 9)
        want = composed_bytes(t, pts, sets, INF)
        before = snapshot()
        assert before["count"].any() and before["framebuffer"].any()
        t.stats()
        got = run(t, dev, pts, sets)
        st = t.stats()
        check(got, want, pts, sets, False, "the visibility bake between the passes")
        assert st["raysTraced"] == st["occludedTraced"] == len(pts) * 65 and st["kernelLaunches"] == 1 and st["stackOverflow"] == 0
        after = snapshot()
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k
        assert t.accumulate(8).tobytes() == want16.tobytes(), "the accumulate pass behind the bake continues the one-shot render"
        assert t.render(16).tobytes() == want16.tobytes(), "the render digest"
        assert t.query_radiance(org, d, 8, seed=5).tobytes() == probes.tobytes()
    finally:
        t.close()


# ----------------------------------------------------------------------------- 8. a moved mesh
def test_a_visibility_bake_sees_the_moved_mesh(dev):
    prt_amd.build()
    scene, _ = HS.scene("plain")
    t = prt_amd.PathTracer(max_depth=8)
    try:
        t.upload_scene(scene)
        pts, sets = VC.make_points("plain", 3), VC.make_sets(3, 65, 1)
        first = run(t, dev, pts, sets)
        moved = (scene.arrays()["meshes"][1]["positions"] + np.array([0.1, 0.05, 0.1], F)).astype(F)  # the tilted patch the points face
        scene.update_positions(1, moved)
        t.update_meshes(scene, [1])
        second = run(t, dev, pts, sets)
        want = composed_bytes(t, pts, sets, INF)
        check(second, want, pts, sets, False, "after update_meshes")
        assert shares(want) >= 0.1 and second[1].tobytes() != first[1].tobytes()
    finally:
        t.close()


# ----------------------------------------------------------------------------- 9. a caller's stream
def test_device_arrays_on_a_callers_stream_with_a_copy_behind(tracers, dev):
    t, _ = tracers("plain")
    pts, sets = VC.make_points("plain", 3), VC.make_sets(3, 130, 9)
    want_out, want_occ = run(t, dev, pts, sets, VC.finite_distance("plain"), triple=True)  # the host route
    words, nbytes = len(want_out), len(want_occ)
    stream = dev.stream()
    d_pts, d_dirs, d_w, d_out, d_copy = (dev.upload(a) for a in (np.zeros_like(pts), sets.dirs, sets.weights, sentinel(words), sentinel(words)))
    d_occ, d_occ_copy = dev.upload(byte_sentinel(nbytes - BYTE_TAIL)), dev.upload(np.zeros(nbytes, np.uint8))
    got, got_occ = np.zeros(words, U), np.zeros(nbytes, np.uint8)
    # the points arrive on the caller's stream, the bake is queued behind them and device copies of both answers behind the bake
    dev.upload_async(pts, stream, d_pts)
    tb = prt_amd.BakeSets(K=sets.K, C=sets.C, nSets=sets.nSets, reserved=0, dirs=d_dirs, weights=d_w)
    t.stats()
    t.bake_visibility_async(len(pts), d_pts, tb, d_out, max_distance=VC.finite_distance("plain"), triple=True, d_occluded=d_occ, stream=stream)
    dev.copy_async(d_copy, d_out, words * 4, stream)
    dev.copy_async(d_occ_copy, d_occ, nbytes, stream)
    dev.download_async(got, d_copy, stream)
    dev.download_async(got_occ, d_occ_copy, stream)
    dev.synchronize(stream)
    assert got.tobytes() == want_out.tobytes() and got_occ.tobytes() == want_occ.tobytes(), "the host route and the device route differ"
    st = t.stats()
    assert st["kernelLaunches"] == 1 and st["raysTraced"] == len(pts) * 130


# ----------------------------------------------------------------------------- 10. end to end
def test_lightmap_visibility_equals_its_parts(tracers):
    t, arrays = tracers("teapot")
    W, H, K, tile, gutter, bias, md = 64, 56, 16, 2, 2, 1e-3, 0.5
    uvs = {}
    for m, mesh in enumerate(arrays):  # each mesh in a half of the atlas, a cell per triangle (tests/test_gpu_atlas.py scene_atlas)
        prims = len(mesh["indices"])
        G = int(np.ceil(np.sqrt(prims)))
        k = np.arange(prims)
        corner = np.array([(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)])
        uv = ((np.stack([k % G, k // G], axis=1).astype(np.float64)[:, None, :] + corner[None]) / G).astype(F)
        uv[:, :, 0] = uv[:, :, 0] * F(0.5) + F(0.5) * m
        uvs[m] = uv
    rng = np.random.default_rng(9)
    made = [prt_amd.bake_cosine_set(K, rng) for _ in range(tile * tile)]
    dirs, weights = np.stack([s[0] for s in made]), np.stack([np.full((K, 1), 1.0 / K, F) for _ in made])  # ambient occlusion
    p = prt_amd.AtlasFilterParams(3, 4, 3.0, 2.0)
    kw = dict(max_distance=md, bias=bias, set_tile=tile, gutter=gutter)
    plain, p_mask = t.lightmap_visibility(uvs, W, H, dirs, weights, **kw)
    filtered, f_mask = t.lightmap_visibility(uvs, W, H, dirs, weights, filter=p, **kw)
    assert plain.shape == (H, W, 1) and filtered.shape == (H, W, 1, 3) and f_mask.tobytes() == p_mask.tobytes()
    # the calls composed here, on host arrays
    texels, hits, counts = t.atlas_rasterize(uvs, W, H)
    assert counts["n"] == len(texels) > 300
    pts = t.atlas_points(texels, hits, W, bias=bias, set_tile=tile)
    ao = t.bake_visibility(pts["P"], pts["N"], dirs, weights, max_distance=md, bias=pts["bias"], sets=pts["set"])
    print(f"ambient occlusion of {len(texels)} texels within {md}: {float((ao == 1).mean()):.3f} of them open, mean {float(ao.mean()):.3f}")
    assert (ao == 1).any() and (ao < 1).any() and ((ao >= 0) & (ao <= 1)).all(), "some texels open, some not (sums of sixteenths are exact)"
    composed, c_mask = t.atlas_resolve(texels, ao, W, H, gutter=gutter)
    BR.same_bytes(plain, composed, "lightmap_visibility() against its four calls")
    assert p_mask.tobytes() == c_mask.tobytes() and set(np.unique(c_mask)) >= {1, 2}, "the mask and the gutter of atlas_resolve as they stand"
    ao3 = t.bake_visibility(pts["P"], pts["N"], dirs, weights, max_distance=md, bias=pts["bias"], sets=pts["set"], triple=True)
    assert ao3.shape == (len(texels), 1, 3) and all(ao3[:, :, h].tobytes() == ao.tobytes() for h in range(3))
    smooth = t.atlas_filter(texels, pts, ao3, W, H, p)
    composed_f, _ = t.atlas_resolve(texels, smooth, W, H, gutter=gutter)
    BR.same_bytes(filtered, composed_f, "lightmap_visibility(filter=p) against its five calls")
    assert filtered.tobytes() != np.repeat(plain[..., None], 3, axis=3).tobytes(), "the filter changed something"
