"""Adaptive sampling on C3 (BASELINE config 3 stand-in: 1920x1080, depth 8): what the machinery costs, what a pass costs against its
active fraction, and the time to a noise target against uniform accumulate passes.  Times are the library's HIP events around each
frame-kernel launch (kernelMsSum of prt_hip_get_stats; the selection is outside them) and the host's wall clock over whole passes
(selection, the pass's one synchronisation, the launch, up to the end of the kernel).  Writes one JSON file stamped with source_sha16
and prints it.

    python tools/adaptive_bench.py [--reps 3] [--cap 2048] [--targets 0.02,0.05,0.1] [--out profiles/r06_adaptive_c3.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prt_amd  # noqa: E402

W, H, DEPTH, FLOOR = 1920, 1080, 8, 0.01


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cap", type=int, default=2048, help="samples per pixel at which the end-to-end runs stop")
    ap.add_argument("--targets", default="0.02,0.05,0.1", help="error targets of the end-to-end runs (95 %% of the pixels at or below)")
    ap.add_argument("--out", default="profiles/r06_adaptive_c3.json")
    args = ap.parse_args()
    prt_amd.build()
    scene, camera, E = prt_amd.setup_atrium_standin(W, H, tris=262000, seed=1)
    t = prt_amd.PathTracer(max_depth=DEPTH)
    t.upload_scene(scene)
    t.set_camera(camera)
    out = {"workload": "c3_sponza_standin", "width": W, "height": H, "max_depth": DEPTH, "floor": FLOOR, "reps": args.reps,
           "source_sha16": prt_amd.loaded_source_sha16(), "device": t.device_info()[0]}

    def timed(fn):
        """(fn's result, wall ms, stats) of queued work, up to the device synchronisation of t.stats()."""
        t.stats()
        t0 = time.perf_counter()
        r = fn()
        st = t.stats()
        return r, (time.perf_counter() - t0) * 1e3, st

    def image():
        img = np.zeros((H, W, 3), dtype=np.float32)
        t._download(img, 0, 0, W - 1, H - 1)
        return img

    # ---- 1. the machinery: 8 adaptive passes of 8 spp with every pixel active against 8 accumulate passes, alternating
    def accumulate_8x8():
        t.accum_reset()
        for _ in range(8):
            t.accumulate_async(8, exposure=E)
        return None

    def adaptive_8x8():
        t.accum_reset()
        return [t.adaptive_pass_async(8, 0.0, 64, 64, FLOOR, exposure=E) for _ in range(8)]

    variants = {"accumulate_8x8": accumulate_8x8, "adaptive_8x8_all_active": adaptive_8x8}
    res = {k: {"kernel": [], "wall": []} for k in variants}
    imgs = {}
    for fn in variants.values():
        timed(fn)  # warm-up: code objects, buffers, the compaction's scratch
    for _ in range(args.reps):
        for name, fn in variants.items():
            r, wall, st = timed(fn)
            res[name]["kernel"].append(st["kernelMsSum"])
            res[name]["wall"].append(wall)
            imgs[name] = image()
            if r is not None:
                assert all(a == W * H for a in r), r
    m = {}
    for name, v in res.items():
        m[name] = {"kernel_ms": med(v["kernel"]), "wall_ms": med(v["wall"]), "kernel_ms_all": [round(x, 3) for x in v["kernel"]],
                   "wall_ms_all": [round(x, 3) for x in v["wall"]]}
    a, b = m["adaptive_8x8_all_active"], m["accumulate_8x8"]
    a["kernel_overhead_frac"] = a["kernel_ms"] / b["kernel_ms"] - 1.0
    a["wall_overhead_frac"] = a["wall_ms"] / b["wall_ms"] - 1.0
    a["image_equals_accumulate"] = bool(imgs["adaptive_8x8_all_active"].tobytes() == imgs["accumulate_8x8"].tobytes())
    out["machinery"] = m

    # ---- 2. selection + read-back of one pass: a pass that selects nobody (min = max = 0: every pixel resolved), call to return
    def selection_ms(n=20):
        for _ in range(3):
            t.adaptive_pass_async(8, 0.0, 0, 0, FLOOR, exposure=E)
        v = []
        for _ in range(n):
            t.stats()
            t0 = time.perf_counter()
            t.adaptive_pass_async(8, 0.0, 0, 0, FLOOR, exposure=E)
            v.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": med(v), "min_ms": float(min(v)), "max_ms": float(max(v)), "calls": n}

    out["selection_readback_1080p"] = selection_ms()

    # ---- 3. one 16-spp pass against its active fraction, from a common 32-spp state (thresholds from accum_error's quantiles; the
    # 100 % row takes minSamples above every count, so that every pixel is traced, those with err 0 included)
    t.accum_reset()
    t.adaptive_pass_async(32, 0.0, 32, 4096, FLOOR, exposure=E)
    err = t.accum_error(E, FLOOR)
    state, mom = t.accum_export(), t.accum_export_moments()
    frac = {}
    for f in (1.0, 0.5, 0.1, 0.01):
        thr = 0.0 if f == 1.0 else float(np.quantile(err, 1.0 - f))
        lo = 4096 if f == 1.0 else 0
        ks, ws, rays, act = [], [], [], []
        for _ in range(args.reps):
            t.accum_import(state)
            t.accum_import_moments(mom)
            active, wall, st = timed(lambda: t.adaptive_pass_async(16, thr, lo, 4096, FLOOR, exposure=E))
            ks.append(st["kernelMsSum"])
            ws.append(wall)
            rays.append(st["raysTraced"] + st["occludedTraced"])
            act.append(active)
        assert len(set(act)) == 1 and len(set(rays)) == 1, (act, rays)
        frac[f"{f:g}"] = {"threshold": thr, "active": act[0], "active_frac": act[0] / (W * H), "kernel_ms": med(ks), "wall_ms": med(ws),
                          "rays": rays[0], "kernel_ms_all": [round(x, 3) for x in ks], "wall_ms_all": [round(x, 3) for x in ws]}
    for v in frac.values():
        v["kernel_ms_over_all_active"] = v["kernel_ms"] / frac["1"]["kernel_ms"]
    out["pass_16spp_by_active_fraction"] = frac

    # ---- 4. end to end: time until 95 % of the pixels have err <= target.  Adaptive: passes at threshold = target from an empty
    # accumulator.  Uniform: plain accumulate passes, as many as the target needs; that number comes from an untimed probe of
    # all-active adaptive passes (minSamples = maxSamples = cap: every pixel traced, the accumulator bit for bit that of the accumulate
    # passes, and the moments kept for the error).  accum_error itself is never timed.
    goal, step = 0.95, 32
    targets = [float(x) for x in args.targets.split(",")]

    def at_target(target):
        return float((t.accum_error(E, FLOOR) <= target).mean())

    t.accum_reset()
    probe = []  # per uniform pass: the fraction of pixels at or below each target
    while len(probe) * step < args.cap:
        t.adaptive_pass_async(step, 0.0, args.cap, args.cap, FLOOR, exposure=E)
        probe.append([at_target(x) for x in targets])
        if all(p >= goal for p in probe[-1]):
            break
    t.accum_reset()
    uni_wall, uni_kernel = [], []
    for _ in probe:
        _, w, st = timed(lambda: t.accumulate_async(step, exposure=E))
        uni_wall.append(w)
        uni_kernel.append(st["kernelMsSum"])
    e2e = {"goal_frac": goal, "step": step, "cap_spp": args.cap, "floor": FLOOR, "targets": {}}
    for i, target in enumerate(targets):
        need = next((k + 1 for k, p in enumerate(probe) if p[i] >= goal), None)
        k = need or len(probe)
        uniform = {"reached": need is not None, "frac_at_target": probe[k - 1][i], "passes": k, "spp": k * step,
                   "wall_ms": float(sum(uni_wall[:k])), "kernel_ms": float(sum(uni_kernel[:k]))}
        t.accum_reset()
        wall = kernel = 0.0
        passes, done, active = 0, 0.0, 1
        while done < goal and active > 0:
            active, w, st = timed(lambda: t.adaptive_pass_async(step, target, step, args.cap, FLOOR, exposure=E))
            wall += w
            kernel += st["kernelMsSum"]
            passes += 1
            done = at_target(target)
        c = t.accum_counts()
        adaptive = {"reached": done >= goal, "frac_at_target": done, "passes": passes, "wall_ms": wall, "kernel_ms": kernel,
                    "mean_spp": float(c.mean()), "max_spp": int(c.max()), "samples_total": int(c.sum(dtype=np.uint64))}
        row = {"adaptive": adaptive, "uniform": uniform}
        if adaptive["reached"] and uniform["reached"]:
            row["wall_speedup"] = uniform["wall_ms"] / adaptive["wall_ms"]
        e2e["targets"][f"{target:g}"] = row
    out["end_to_end"] = e2e

    # ---- 2b. the same selection at 4K: C3's camera at 3840x2160 (the camera does not depend on the mesh), empty accumulator
    t.set_camera(prt_amd.setup_atrium_standin(3840, 2160, tris=2000, seed=1)[1])
    out["selection_readback_4k"] = selection_ms()
    t.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
