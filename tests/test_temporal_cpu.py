"""Temporal reprojection without a GPU: the product exports the entry points, the header documents them and carries the rules of the
stage (include/prt_hip.h "temporal reprojection"), Python binds them, the compiled merge kernel uses no scratch, no LDS and at most
64 registers, the position kernel is no heavier than the G-buffer kernel, and the numpy restatement the GPU tests compare against
(prt_temporal_ref) gives, on hand-made cases, the answer a plain per-pixel loop works out."""
import os
import re
import subprocess

import numpy as np
import pytest

import prt_amd
import prt_denoise_ref as R
import prt_temporal_ref as TR
import prt_testlib as T
from prt_amd import _build as B
from prt_testlib import bits

F = np.float32
ENTRY_POINTS = ("prt_hip_denoise_get_position", "prt_hip_denoise_set_position", "prt_hip_accum_denoise_temporal", "prt_hip_history_reset",
                "prt_hip_history_export", "prt_hip_history_import")


@pytest.fixture(scope="module")
def L():
    prt_amd.build()
    return prt_amd.lib()


def test_product_exports_the_temporal_entry_points(L):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", prt_amd.LIB_PATH]).decode()
    for name in ENTRY_POINTS:
        assert re.search(rf" T {name}$", syms, re.M), name
        assert name in prt_amd.EXPORTS, name
        assert hasattr(L, name), name
    assert not re.search(r"prt_hip_test_temporal_profile", syms)  # test library only


def test_header_documents_the_stage():
    src = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", src), name
    block = src[src.index("temporal reprojection"):]
    assert "prt_temporal_params" in block
    for rule in ("dot3(u, w) = (u.x*w.x + u.y*w.y) + u.z*w.z",
                 "kAspect = (float)W / (float)H",
                 "nx = 2.0f * ((float)x * invWidth - 0.5f + 0.0f) * 0.6f * kAspect",
                 "ny = -2.0f * ((float)y * invHeight - 0.5f + 0.0f) * 0.6f",
                 "v = (nx*right + ny*up) + dir per component",
                 "dirp = (1.0f / sqrtf((v.x*v.x + v.y*v.y) + v.z*v.z)) * v",
                 "maxT = 100000.0f", "X = pos + t*dirp per component", "a miss is {0, 0, 0, -1}",
                 "{hC.xyz, hV}, {hX.xyz, hLen}, {hN.xyz, 0}",
                 "if valid_p and t_p >= 0 and a history exists and maxHistory > 0:",
                 "e = X_p - hc.pos;  a = dot3(e, hc.right);  b = dot3(e, hc.up);  z = dot3(e, hc.dir)",
                 "if z > 0:",
                 "fx = ((a / z) / ((2.0f*0.6f) * kAspect) + 0.5f) * (float)W",
                 "fy = (0.5f - (b / z) / (2.0f*0.6f)) * (float)H",
                 "if fx >= -1.0f and fx < (float)W and fy >= -1.0f and fy < (float)H:", "(false for NaN)",
                 "ix = floorf(fx); iy = floorf(fy); tx = fx - ix; ty = fy - iy",
                 "lim = (positionTolerance*positionTolerance) * (t_p*t_p)",
                 "taps q = (ix + i, iy + j), j = 0,1 outer, i = 0,1 inner; skipped when outside the image or !(hLen_q > 0)",
                 "g = X_p - hX_q;  accepted iff dot3(g, g) <= lim and dot3(N_p, hN_q) >= normalCos",
                 "wb = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty)",
                 "sumW += wb; sumC += wb * hC_q (per channel); sumL += wb * hLen_q",
                 "if hV_q >= 0: sumVh += wb * hV_q; sumWv += wb",
                 "have = sumW > 0.015625f",
                 "Hc = sumC / sumW;  q = sumL / sumW;  Hl = q < maxHistory ? q : maxHistory;  Hv = sumWv > 0 ? sumVh / sumWv : -1",
                 "n = (float)count_p;  tot = n + Hl",
                 "cm = (n * c_p + Hl * Hc) / tot",
                 "vm = v_p >= 0 and Hv >= 0 ? ((n*n)*v_p + (Hl*Hl)*Hv) / (tot*tot)",
                 ": v_p >= 0 ? (v_p * n) / tot", ": Hv  >= 0 ? (Hv * Hl) / tot",
                 "cm = c_p;  vm = v_p;  len = valid_p ? (float)count_p : 0",
                 "demodulate: C0_p = cm / d_p (per channel);  V0_p = vm < 0 ? -1 : vm / (lum(d_p)*lum(d_p))",
                 "otherwise:  C0_p = cm;  V0_p = vm",
                 "pending_p = {cm, vm}, {X_p, (valid_p and t_p >= 0) ? len : 0}, {N_p, 0};  pending camera = the current camera",
                 "RADIANCE space", "never with pending", "promotes it to history", "prt_hip_history_reset drop both",
                 "prt_hip_accum_reset / prt_hip_accum_import touch neither", "BIASED for view-dependent radiance",
                 "varying `seed` per view", "16 bytes (position) plus 2 x 48 bytes", "no FMA", "PRT_HIP_ESTATE", "PRT_HIP_EINVAL",
                 "A tap with a NaN hLen is skipped", "A NaN hV is not summed", "takes the next branch of vm",
                 "A non-finite history colour enters every merged pixel\n * whose accepted bilinear taps include it",
                 "carried in the pending record into the next history", "prt_hip_history_reset ends this"):
        assert rule in block, rule


def test_python_host_binds_the_temporal_api():
    assert [n for n, _ in prt_amd.TemporalParams._fields_] == ["positionTolerance", "normalCos", "maxHistory"]
    for m in ("denoise_temporal", "denoise_temporal_async", "denoise_position", "set_denoise_position", "history_reset", "history_export",
              "history_import"):
        assert callable(getattr(prt_amd.PathTracer, m)), m
    assert "prt_temporal.hip" in B.SOURCES
    t = prt_amd.PathTracer.temporal_params()
    assert (t.positionTolerance, t.normalCos, t.maxHistory) == (F(0.01), F(0.9), 256.0)


def kernel_resources(source):
    """{kernel name: {VGPRs, ScratchSize, ...}} of one translation unit, from the compiler's resource-usage remarks (product flags)."""
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC", "-pthread", "-ldl")]
    cmd = [B.hipcc()] + flags + ["--cuda-device-only", "-c", os.path.join(B.CSRC, source), "-o", os.devnull,
                                 "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, check=True).stderr
    out, cur = {}, None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
        elif cur is not None:
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
            if m:
                cur[m.group(1).strip()] = int(m.group(2))
    return out


def test_temporal_kernel_resources():
    res = kernel_resources("prt_temporal.hip")
    merge = [r for k, r in res.items() if "tp_merge_kernel" in k]
    position = [r for k, r in res.items() if "position_kernel" in k]
    assert len(merge) == 1 and len(position) == 1, list(res)
    m, p = merge[0], position[0]
    print("tp_merge_kernel", m)
    print("position_kernel", p)
    assert m["ScratchSize"] == 0 and m["VGPRs"] <= 64 and m["Occupancy"] == 8 and m["LDS Size"] == 0, m
    g = [r for k, r in kernel_resources("prt_kernels.hip").items() if "gbuffer_kernel" in k]
    assert len(g) == 1
    print("gbuffer_kernel", g[0])
    assert p["ScratchSize"] <= g[0]["ScratchSize"] and p["Occupancy"] >= g[0]["Occupancy"] and p["VGPRs"] <= g[0]["VGPRs"], (p, g[0])


# ---- the restatement against a plain loop: one pixel at a time, float32 operations in the header's order, python bookkeeping
def loop_merge(total, count, mom, albedo, normal, position, history, tol, ncos, maxh):
    h, w = count.shape
    tol, ncos, maxh = F(tol), F(ncos), F(maxh)
    out = dict(cm=np.zeros((h, w, 3), F), vm=np.zeros((h, w), F), len=np.zeros((h, w), F), have=np.zeros((h, w), bool),
               sum_w=np.zeros((h, w), F), fx=np.full((h, w), np.nan, F), fy=np.full((h, w), np.nan, F), plen=np.zeros((h, w), F))

    def dot(u, v):
        return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]

    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                cnt = int(count[y, x])
                valid = cnt > 0
                G = [F(g) for g in normal[y, x]]
                N = [F(0)] * 3 if all(g == 0 for g in G) else [(g - F(0.5)) * F(2.0) for g in G]
                n = F(cnt)
                c = [F(s) / n for s in total[y, x]] if valid else [F(0)] * 3
                m = int(mom[y, x, 2:3].view(np.uint32)[0])
                v = (F(mom[y, x, 1]) / F(m - 1)) / F(cnt >> 3) if valid and m >= 2 else F(-1)
                X = [F(a) for a in position[y, x, :3]]
                t = F(position[y, x, 3])
                have = False
                sw = sl = svh = swv = F(0)
                sc = [F(0)] * 3
                if valid and t >= 0 and history is not None and maxh > 0:
                    hc = TR.camera_fields(history["camera"])
                    e = [X[k] - hc["pos"][k] for k in range(3)]
                    a, b, z = dot(e, hc["right"]), dot(e, hc["up"]), dot(e, hc["dir"])
                    if z > 0:
                        ka = F(w) / F(h)
                        fx = ((a / z) / ((F(2.0) * F(0.6)) * ka) + F(0.5)) * F(w)
                        fy = (F(0.5) - (b / z) / (F(2.0) * F(0.6))) * F(h)
                        out["fx"][y, x], out["fy"][y, x] = fx, fy
                        if fx >= F(-1.0) and fx < F(w) and fy >= F(-1.0) and fy < F(h):
                            ix, iy = np.floor(fx), np.floor(fy)
                            tx, ty = fx - ix, fy - iy
                            lim = (tol * tol) * (t * t)
                            for j in (0, 1):
                                for i in (0, 1):
                                    qx, qy = int(ix) + i, int(iy) + j
                                    if qx < 0 or qy < 0 or qx >= w or qy >= h:
                                        continue
                                    hl = F(history["pos_len"][qy, qx, 3])
                                    if not hl > 0:
                                        continue
                                    g = [X[k] - F(history["pos_len"][qy, qx, k]) for k in range(3)]
                                    hn = [F(a) for a in history["normal"][qy, qx, :3]]
                                    if not (dot(g, g) <= lim and dot(N, hn) >= ncos):
                                        continue
                                    wb = (tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)
                                    sw = sw + wb
                                    sc = [sc[k] + wb * F(history["color_var"][qy, qx, k]) for k in range(3)]
                                    sl = sl + wb * hl
                                    hv = F(history["color_var"][qy, qx, 3])
                                    if hv >= 0:
                                        svh = svh + wb * hv
                                        swv = swv + wb
                            have = bool(sw > F(0.015625))
                out["sum_w"][y, x] = sw
                if have:
                    Hc = [s / sw for s in sc]
                    q = sl / sw
                    Hl = q if q < maxh else maxh
                    Hv = svh / swv if swv > 0 else F(-1)
                    tot = n + Hl
                    cm = [(n * c[k] + Hl * Hc[k]) / tot for k in range(3)]
                    if v >= 0 and Hv >= 0:
                        vm = ((n * n) * v + (Hl * Hl) * Hv) / (tot * tot)
                    elif v >= 0:
                        vm = (v * n) / tot
                    elif Hv >= 0:
                        vm = (Hv * Hl) / tot
                    else:
                        vm = F(-1)
                    ln = tot
                else:
                    cm, vm, ln = c, v, (n if valid else F(0))
                out["cm"][y, x], out["vm"][y, x], out["len"][y, x], out["have"][y, x] = cm, vm, ln, have
                out["plen"][y, x] = ln if (valid and t >= 0) else F(0)
    return out


def camera(pos, direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), right=(1.0, 0.0, 0.0), width=12, height=8):
    return dict(pos=pos, dir=direction, up=up, right=right, invWidth=F(1.0) / F(width), invHeight=F(1.0) / F(height))


W, H, DEPTH = 12, 8, 2.0


def plane_seen_from(cam, z_plane=-DEPTH):
    """The position plane of a camera looking down -z at the plane z = z_plane."""
    d = TR.centre_directions(cam, W, H)
    t = ((F(z_plane) - F(cam["pos"][2])) / d[..., 2]).astype(F)
    return TR.position_plane(cam, W, H, t)


def scene(seed=1, hist_cam=None, cur_cam=None):
    rng = np.random.default_rng(seed)
    cur_cam = cur_cam or camera((0.0, 0.0, 0.0))
    hist_cam = hist_cam or cur_cam
    count = np.full((H, W), 8, np.uint32)
    total = (rng.random((H, W, 3)) * 8).astype(F)
    mom = np.zeros((H, W, 4), F)
    mom[..., 1] = rng.random((H, W)).astype(F)
    mom[..., 2] = np.full((H, W), 2, np.uint32).view(F)
    albedo = np.full((H, W, 3), 0.5, F)
    normal = np.zeros((H, W, 3), F)
    normal[...] = (0.5, 0.5, 1.0)  # +z
    pos = plane_seen_from(cur_cam)
    hpos = plane_seen_from(hist_cam)
    hist = dict(camera=hist_cam,
                color_var=np.concatenate([rng.random((H, W, 3)), rng.random((H, W, 1)) * 0.1], -1).astype(F),
                pos_len=np.concatenate([hpos[..., :3], np.full((H, W, 1), 64.0)], -1).astype(F),
                normal=np.concatenate([np.zeros((H, W, 2)), np.ones((H, W, 1)), np.zeros((H, W, 1))], -1).astype(F))
    return dict(total=total, count=count, mom=mom, albedo=albedo, normal=normal, position=pos), hist


def both(state, hist, tol=0.01, ncos=0.9, maxh=256.0):
    want = loop_merge(history=hist, tol=tol, ncos=ncos, maxh=maxh, **state)
    got = TR.merge(history=hist, position_tolerance=tol, normal_cos=ncos, max_history=maxh, **state)
    assert (got["have"] == want["have"]).all()
    for k in ("cm", "vm", "len"):
        assert (bits(got[k]) == bits(want[k])).all(), k
    assert (bits(got["pending"][0][..., :3]) == bits(want["cm"])).all() and (bits(got["pending"][0][..., 3]) == bits(want["vm"])).all()
    assert (bits(got["pending"][1][..., 3]) == bits(want["plen"])).all()
    assert (bits(got["pending"][1][..., :3]) == bits(state["position"][..., :3])).all()
    return want


def test_same_camera_reprojects_every_pixel_onto_itself():
    state, hist = scene()
    r = both(state, hist)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    assert np.abs(r["fx"] - xs).max() < 1e-3 and np.abs(r["fy"] - ys).max() < 1e-3
    assert r["have"].all() and (r["len"] == 72).all()
    # the neighbours are a pixel footprint (0.1 * t) away, far beyond 0.01 * t: the pixel's own tap is the only one
    n, hl = 8.0, 64.0
    c = state["total"].astype(np.float64) / n
    assert np.allclose(r["cm"], (n * c + hl * hist["color_var"][..., :3]) / (n + hl), rtol=1e-5, atol=0)
    v = state["mom"][..., 1].astype(np.float64)  # M2 / (2 - 1) / (8 >> 3)
    assert np.allclose(r["vm"], (n * n * v + hl * hl * hist["color_var"][..., 3]) / (n + hl) ** 2, rtol=1e-5, atol=0)


def test_one_pixel_sideways_shift():
    """The history camera stands one pixel footprint to the left: what the current pixel x sees was history pixel x + 1."""
    foot = 2.0 * 0.6 * (W / H) * DEPTH / W
    state, hist = scene(hist_cam=camera((-foot, 0.0, 0.0)))
    r = both(state, hist)
    xs, _ = np.meshgrid(np.arange(W), np.arange(H))
    assert np.abs(r["fx"] - (xs + 1)).max() < 1e-3
    assert r["have"][:, :W - 1].all() and not r["have"][:, W - 1].any()  # the last column left the history's image
    c = state["total"][:, :W - 1].astype(np.float64) / 8.0
    assert np.allclose(r["cm"][:, :W - 1], (8.0 * c + 64.0 * hist["color_var"][:, 1:, :3]) / 72.0, rtol=1e-5, atol=0)
    assert (bits(r["cm"][:, W - 1]) == bits((state["total"][:, W - 1] / F(8)).astype(F))).all()


def test_rejections_and_special_cases():
    state, hist = scene(seed=2)
    hist["pos_len"][1, 1, 2] += F(0.05)          # 0.05 > 0.01 * t (t ~ 2): rejected by distance
    hist["normal"][2, 2, :3] = (1.0, 0.0, 0.0)   # rejected by normal
    hist["pos_len"][3, 3, 3] = 0.0               # hLen = 0
    state["position"][4, 4, :3] = np.nan         # NaN position with t >= 0
    state["position"][5, 5] = (0, 0, 0, -1)      # the centre ray missed
    state["count"][6, 6] = 0                     # invalid
    state["total"][6, 6] = 0
    state["position"][0, 7, 3] = np.nan          # NaN t
    hist["pos_len"][7, 8, :3] = np.nan           # NaN in the history
    r = both(state, hist)
    for y, x in ((1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (0, 7), (7, 8)):
        assert not r["have"][y, x], (y, x)
    assert r["have"].sum() == W * H - 8
    assert r["plen"][5, 5] == 0 and r["plen"][6, 6] == 0 and r["plen"][0, 7] == 0 and r["plen"][4, 4] == 8 and r["plen"][1, 1] == 8
    assert (r["cm"][6, 6] == 0).all() and r["vm"][6, 6] == -1 and r["len"][6, 6] == 0
    # the history behind the camera (z <= 0), and a history camera that looks elsewhere (fx outside the image)
    state, hist = scene(seed=3, hist_cam=camera((0.0, 0.0, -2.0 * DEPTH), direction=(0.0, 0.0, -1.0)))
    r = both(state, hist)
    assert not r["have"].any() and np.isnan(r["fx"]).all()
    state, hist = scene(seed=3, hist_cam=camera((0.0, 0.0, -DEPTH)))  # z == 0 exactly
    assert not both(state, hist)["have"].any()
    state, hist = scene(seed=4, hist_cam=camera((-10.0, 0.0, 0.0)))
    r = both(state, hist)
    assert not r["have"].any() and (r["fx"] >= W).all()
    state, hist = scene(seed=4, hist_cam=camera((10.0, 0.0, 0.0)))
    r = both(state, hist)
    assert not r["have"].any() and (r["fx"] < -1).all()
    # no history at all
    state, _ = scene(seed=5)
    r = both(state, None)
    assert not r["have"].any() and (r["len"] == 8).all()


def test_the_four_variance_cases_and_the_cap():
    state, hist = scene(seed=6)
    m = state["mom"][..., 2].view(np.uint32)
    m[:, :W // 2] = 1                       # left half: the pixel's own variance unknown
    hist["color_var"][:H // 2, :, 3] = -1   # top half: the history's variance unknown
    r = both(state, hist)
    n, hl, tot = F(8), F(64), F(72)
    v = state["mom"][..., 1]
    hv = hist["color_var"][..., 3]
    top, left = np.zeros((H, W), bool), np.zeros((H, W), bool)
    top[:H // 2], left[:, :W // 2] = True, True
    assert (r["vm"][top & left] == -1).all()
    assert np.allclose(r["vm"][top & ~left], (v * n / tot)[top & ~left], rtol=1e-6)
    assert np.allclose(r["vm"][~top & left], (hv * hl / tot)[~top & left], rtol=1e-5)
    assert np.allclose(r["vm"][~top & ~left], ((n * n * v + hl * hl * hv) / (tot * tot))[~top & ~left], rtol=1e-5)
    # maxHistory caps the length the history stands for, and 0 switches the merge off
    hist["pos_len"][..., 3] = 1000.0
    r = both(state, hist, maxh=256.0)
    assert (r["len"] == 264).all()
    r = both(state, hist, maxh=32.0)
    assert (r["len"] == 40).all()
    c = state["total"].astype(np.float64) / 8.0
    assert np.allclose(r["cm"], (8.0 * c + 32.0 * hist["color_var"][..., :3]) / 40.0, rtol=1e-5, atol=0)
    r = both(state, hist, maxh=0.0)
    assert not r["have"].any() and (r["len"] == 8).all()


def test_sum_of_weights_just_below_and_above_one_64th():
    """The history camera stands a fraction d of a pixel footprint to the left and above, so that every pixel falls between four
    history pixels with tx = ty = d, and only history pixel (4, 4) stands for any samples.  For the current pixel (3, 3) it is the
    (1, 1) tap, whose weight is d * d: 0.0144 for d = 0.12, 0.0169 for d = 0.13, either side of 1/64 = 0.015625."""
    foot_x = 2.0 * 0.6 * (W / H) * DEPTH / W
    foot_y = 2.0 * 0.6 * DEPTH / H
    for d, expect in ((0.12, False), (0.13, True)):
        # current pixel (x, y) lands at history (x + d, y + d): the history camera stands d footprints to the left and d above
        state, hist = scene(seed=7, hist_cam=camera((-d * foot_x, d * foot_y, 0.0)))
        r0 = both(state, hist, tol=1.0)
        xs, ys = np.meshgrid(np.arange(W), np.arange(H))
        assert np.abs(r0["fx"] - (xs + d)).max() < 1e-3 and np.abs(r0["fy"] - (ys + d)).max() < 1e-3
        keep = hist["pos_len"][4, 4, 3]
        hist["pos_len"][..., 3] = 0.0
        hist["pos_len"][4, 4, 3] = keep
        r = both(state, hist, tol=1.0)
        assert abs(float(r["sum_w"][3, 3]) - d * d) < 1e-4 and (r["sum_w"][3, 3] > F(0.015625)) == expect
        assert bool(r["have"][3, 3]) == expect
        assert r["have"].sum() == (4 if expect else 3)  # (4, 4) itself (weight (1-d)^2), (3, 4) and (4, 3) (weight d(1-d)); and (3, 3)
        if expect:
            assert r["len"][3, 3] == 72


def test_whole_restatement_without_history_is_the_plain_denoiser():
    """denoise_temporal(history = None) = prt_denoise_ref.denoise, bit for bit, with and without demodulation."""
    rng = np.random.default_rng(11)
    h, w = 9, 14
    count = (rng.integers(0, 4, (h, w)) * 8).astype(np.uint32)
    total = (rng.random((h, w, 3)) * count[..., None]).astype(F)
    mom = np.zeros((h, w, 4), F)
    mom[..., 1] = rng.random((h, w)).astype(F)
    mom[..., 2] = np.minimum(rng.integers(0, 4, (h, w)), count >> 3).astype(np.uint32).view(F)
    albedo = rng.random((h, w, 3)).astype(F)
    normal = (0.5 + 0.5 * rng.random((h, w, 3))).astype(F)
    normal[0, 0] = 0
    position = rng.random((h, w, 4)).astype(F)
    for demodulate in (True, False):
        img, var, pend = TR.denoise_temporal(total, count, mom, albedo, normal, position, None, iterations=3, demodulate=demodulate,
                                             exposure=0.5)
        want, want_var = R.denoise(total, count, mom, albedo, normal, iterations=3, demodulate=demodulate, exposure=0.5)
        assert (bits(img) == bits(want)).all() and (bits(var) == bits(want_var)).all()
        assert (pend["pos_len"][..., 3] == np.where(position[..., 3] >= 0, count, 0)).all()
