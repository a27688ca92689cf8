"""The oracle's answer to a radiance query (include/prt_hip.h "radiance"): probe q is pixel (0, 0) of orc_trace_block under the
degenerate camera pos = org[q], dir = dir[q], up = right = 0, 1 x 1, and the seed seed + q.  tests/test_probe_cpu.py pins this helper
against OracleScene.trace_block; tests/test_gpu_probe.py holds the product to it at tolerance 0.  Nothing here is product code."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import prt_testlib as T

F = np.float32
# orc_camera / prt DevCamera: pos, dir, up, right, width, height, invWidth, invHeight
CAMERA_DTYPE = np.dtype([("pos", "<f4", 3), ("dir", "<f4", 3), ("up", "<f4", 3), ("right", "<f4", 3), ("width", "<u4"), ("height", "<u4"),
                         ("invWidth", "<f4"), ("invHeight", "<f4")])
assert CAMERA_DTYPE.itemsize == C.sizeof(T.OrcCamera)
MAX_WORKERS = 16


def degenerate_cameras(org, dir):
    """(n,) CAMERA_DTYPE: the camera of every probe, org and dir copied bit for bit (NaN payloads included)."""
    o = np.ascontiguousarray(org, dtype=F).reshape(-1, 3)
    d = np.ascontiguousarray(dir, dtype=F).reshape(-1, 3)
    assert len(o) == len(d)
    cams = np.zeros(len(o), dtype=CAMERA_DTYPE)
    cams["pos"], cams["dir"] = o, d
    cams["width"] = cams["height"] = 1
    cams["invWidth"] = cams["invHeight"] = 1.0
    return cams


def product_camera(org, dir):
    """The same camera for prt_hip_set_camera: a prt_amd.Camera whose desc is filled by hand (Camera.create would build a basis)."""
    import prt_amd
    cam = prt_amd.Camera()
    assert C.sizeof(cam.desc) == CAMERA_DTYPE.itemsize
    C.memmove(C.byref(cam.desc), degenerate_cameras([org], [dir]).tobytes(), CAMERA_DTYPE.itemsize)
    return cam


def trace(osc, org, dir, spp, depth, seed, exposure=1.0, workers=None, which=None):
    """Radiance (n, 3) float32 and the summed (raysTraced, occludedTraced) of the probes (org[q], dir[q]) of OracleScene `osc`, one
    orc_trace_block per probe.  which: only these probe indices are traced (the other rows stay 0, the sums cover `which`)."""
    L = osc.L
    cams = degenerate_cameras(org, dir)
    n = len(cams)
    idx = np.arange(n) if which is None else np.asarray(which, dtype=np.int64)
    out = np.zeros((n, 3), dtype=F)
    stats = (T.OrcStats * len(idx))()
    cam_base, out_base = cams.ctypes.data, out.ctypes.data
    cam_p = C.POINTER(T.OrcCamera)

    def run(lo, hi):
        for k in range(lo, hi):
            q = int(idx[k])
            L.orc_trace_block(osc.scene, C.cast(cam_base + CAMERA_DTYPE.itemsize * q, cam_p), 0, 0, 0, 0, spp, depth, (seed + q) & 0xffffffff,
                              exposure, out_base + 12 * q, C.byref(stats[k]))

    m = len(idx)
    w = min(MAX_WORKERS, workers or MAX_WORKERS, max(1, m // 256))
    if w <= 1:
        run(0, m)
    else:  # ctypes releases the GIL around the call
        step = (m + w - 1) // w
        with ThreadPoolExecutor(max_workers=w) as ex:
            list(ex.map(lambda lo: run(lo, min(m, lo + step)), range(0, m, step)))
    rays = sum(int(s.raysTraced) for s in stats)
    occl = sum(int(s.occludedTraced) for s in stats)
    assert all(int(s.nPx) == 1 for s in stats)
    return out, rays, occl


def fan(center_dir, n, spread, rng):
    """n unnormalised float32 directions around center_dir."""
    c = np.asarray(center_dir, dtype=np.float64)
    d = c[None, :] + rng.uniform(-spread, spread, size=(n, 3))
    return (d * rng.uniform(0.5, 3.0, size=(n, 1))).astype(F)


def stage_probes(n, seed=1):
    """(org, dir) of n probes inside the stage of prt_hostile_shade (x in [-3, 3], floor y = 0, patches at z = 0, wall at z = -2):
    origins jittered above the floor in front of the patches, directions fanned around the stage camera's."""
    import prt_hostile_shade as HS
    rng = np.random.default_rng(seed)
    org = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.3, 1.5, n), rng.uniform(0.5, 3.0, n)], axis=1).astype(F)
    return org, fan(HS.STAGE_CAMERA[1], n, 0.5, rng)


def box_probes(n, seed=2):
    """(org, dir) of n probes inside the closed box of prt_hostile_shade ([-1, 1]^3), any direction."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.8, 0.8, size=(n, 3)).astype(F), fan((0.0, -0.2, -1.0), n, 1.0, rng)


NAN_PAYLOAD = 0xffc12345
# name -> (org or None = the ordinary origin `at`, dir); DEGENERATE: the direction normalises to zero or to non-finite components
HOSTILE = ("zero_dir", "nan_org", "nan_dir", "inf_dir", "huge_dir", "tiny_dir", "neg_zero", "neg_zero_axis", "on_surface", "inside")
DEGENERATE = ("zero_dir", "nan_dir", "inf_dir", "huge_dir", "tiny_dir")


def hostile_probes(at, towards, on_surface, inside):
    """(org (10, 3), dir (10, 3)) of HOSTILE: `at` an ordinary origin, `towards` an ordinary direction, on_surface = (a point of a
    surface, a direction leaving it), inside = (a point no ray leaves the scene from, a direction)."""
    nan = np.array([NAN_PAYLOAD], dtype=np.uint32).view(F)[0]
    t = np.asarray(towards, dtype=F)
    rows = {
        "zero_dir": (at, (0.0, 0.0, 0.0)),
        "nan_org": ((at[0], nan, at[2]), t),
        "nan_dir": (at, (t[0], t[1], nan)),
        "inf_dir": (at, (t[0], -np.inf, t[2])),
        "huge_dir": (at, (0.0, -1e20, -3e20)),       # squared length overflows: normalises to 0
        "tiny_dir": (at, (0.0, -3e-31, -1e-30)),     # squared length underflows to 0: 0 / 0
        "neg_zero": (at, (-0.0, t[1], t[2])),
        "neg_zero_axis": (at, (-0.0, -0.0, -1.0)),
        "on_surface": on_surface,
        "inside": inside,
    }
    org = np.zeros((len(HOSTILE), 3), dtype=F)
    d = np.zeros((len(HOSTILE), 3), dtype=F)
    for k, name in enumerate(HOSTILE):
        org[k], d[k] = np.asarray(rows[name][0], dtype=F), np.asarray(rows[name][1], dtype=F)
    assert org[1].view(np.uint32)[1] == NAN_PAYLOAD and d[2].view(np.uint32)[2] == NAN_PAYLOAD  # the payloads survive
    return org, d


def hostile_case(name):
    """(OracleScene or its desc, org, dir, index of each hostile probe) of one batch of 64: HOSTILE interleaved with ordinary probes."""
    if name == "plain":
        org, d = stage_probes(64, seed=9)
        # from (0.05, 0.5, 2): towards the lit floor; along -z the middle patch; from the floor itself the back wall; from behind the patches
        horg, hd = hostile_probes((0.05, 0.5, 2.0), (0.1, -0.6, -1.0), on_surface=((0.5, 0.0, 1.0), (0.0, 0.15, -1.0)),
                                  inside=((0.0, 0.3, 0.0), (0.0, -0.2, 1.0)))
    else:
        org, d = box_probes(64, seed=9)
        horg, hd = hostile_probes(org[0], d[0], on_surface=((-1.0, 0.2, 0.1), (1.0, -0.3, 0.2)), inside=((0.0, 0.0, 0.0), (0.3, 1.0, -0.2)))
    at = 3 + 6 * np.arange(len(HOSTILE))
    org[at], d[at] = horg, hd
    return org, d, at
