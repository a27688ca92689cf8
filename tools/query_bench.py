"""Ray queries on C3's first-hit rays: the 1920x1080 pixel-centre rays of the bench camera (prt_amd.pixel_centre_rays, the rays
PathTracer.pick shoots) against the C3 stand-in scene, tMax = 100000.  Kernel times (HIP events around the launch, read back through
prt_hip_get_stats) of
    prt_hip_query_nearest            against the test build's prt_hip_trace_rays mode 0 (the same loop behind 2 x 12-byte ray loads, one
                                     workgroup per 1024 rays) on the same rays and the same limit
    prt_hip_query_any                against mode 2
    prt_hip_query_nearest + surfaces against prt_hip_query_nearest alone
after two warm-up calls, `reps` repetitions each, interleaved; median and spread (min, max) and the ratios of the medians.  Runs in
the TEST build of the library, which holds both sides.  Prints one JSON document stamped with source_sha16; --out F also writes it to F.

    python tools/query_bench.py [--reps 7] [--size 1920x1080] [--out F]

--radiance: prt_hip_query_radiance instead.  Probes = pixel-centre rays of the same camera at equal strides over the image, 8 spp,
depth 8: n = 4096 and 262 144 probes in ONE call each (kernel time from prt_hip_get_stats and wall time of the whole host call, staging
included), against the only path there was before -- per probe prt_hip_set_camera with the degenerate 1 x 1 camera, a one-pixel
prt_hip_render under seed + q and a download -- timed by the wall clock over 256 probes and scaled linearly to n (256 calls in a row
cost 256 times one call: nothing is shared between them).  The 256 probes must agree bit for bit between the two paths.

    python tools/query_bench.py --radiance [--reps 7] [--out F]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prt_amd  # noqa: E402


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def emit(out, path):
    text = json.dumps(out, indent=1)
    print(text)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")


def radiance(args):
    W, H = (int(v) for v in args.size.split("x"))
    spp, depth, seed, per_camera = 8, 8, 12345, 256
    scene, camera, _ = prt_amd.setup_atrium_standin(W, H, tris=262000, seed=1)
    t = prt_amd.PathTracer(max_depth=depth, seed=seed)
    t.upload_scene(scene)

    def probes(n):
        idx = (np.arange(n, dtype=np.uint64) * np.uint64(W * H) // np.uint64(n)).astype(np.uint32)
        ys, xs = np.divmod(idx, np.uint32(W))
        r = prt_amd.pixel_centre_rays(camera.desc, xs, ys)
        return r["org"], r["dir"]

    out = {"workload": "c3_sponza_standin", "probes_from": args.size + " pixel-centre rays at equal strides", "spp": spp, "max_depth": depth,
           "reps": args.reps, "device": t.device_info()[0], "compute_units": t.device_info()[1],
           "source_sha16": prt_amd.loaded_source_sha16(), "query": {}}
    answers = {}
    for n in (4096, 262144):
        org, d = probes(n)
        kernel, wall, rays = [], [], 0
        for rep in range(2 + args.reps):
            t0 = time.perf_counter()
            answers[n] = t.query_radiance(org, d, spp)
            dt = (time.perf_counter() - t0) * 1e3  # (includes prt_hip_get_stats: one synchronisation that the call has made already)
            if rep >= 2:
                kernel.append(t.last_stats["kernelMs"])
                wall.append(dt)
            rays = t.last_stats["raysTraced"]
        out["query"][str(n)] = {"kernel_ms": spread(kernel), "wall_ms": spread(wall), "rays_traced": rays,
                                "lit_fraction": float((answers[n] != 0).any(axis=1).mean()),
                                "mprobes_per_s_kernel": n / float(np.median(kernel)) / 1e3}
    # the per-camera path on the first 256 probes of the 4096
    org, d = probes(4096)
    cam = prt_amd.Camera()
    cam.desc.width = cam.desc.height = 1
    cam.desc.invWidth = cam.desc.invHeight = 1.0
    got = np.zeros((per_camera, 3), dtype=np.float32)
    walls = []
    for rep in range(1 + args.reps):
        t0 = time.perf_counter()
        for q in range(per_camera):
            C.memmove(cam.desc.pos, org[q].ctypes.data, 12)
            C.memmove(cam.desc.dir, d[q].ctypes.data, 12)
            t.seed = (seed + q) & 0xffffffff
            t.set_camera(cam)
            got[q] = t.render(spp).reshape(3)
        if rep >= 1:
            walls.append((time.perf_counter() - t0) * 1e3)
    t.seed = seed
    per_probe = float(np.median(walls)) / per_camera
    out["per_camera"] = {"probes": per_camera, "wall_ms": spread(walls), "wall_ms_per_probe": per_probe,
                         "answers_equal_the_query": got.tobytes() == answers[4096][:per_camera].tobytes()}
    out["per_camera_scaled"] = {str(n): {"wall_ms": per_probe * n, "scaling": f"{per_camera} probes measured, times {n}/{per_camera}",
                                         "over_query_wall": per_probe * n / out["query"][str(n)]["wall_ms"]["median"]} for n in (4096, 262144)}
    t.close()
    emit(out, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--out", default=None)
    ap.add_argument("--radiance", action="store_true")
    args = ap.parse_args()
    prt_amd.build()
    if args.radiance:
        return radiance(args)
    W, H = (int(v) for v in args.size.split("x"))
    scene, camera, _ = prt_amd.setup_atrium_standin(W, H, tris=262000, seed=1)
    t = prt_amd.PathTracer(max_depth=8, test_entry_points=True)
    t.upload_scene(scene)
    ys, xs = np.divmod(np.arange(W * H, dtype=np.uint32), np.uint32(W))
    rays = prt_amd.pixel_centre_rays(camera.desc, xs, ys)
    org, d, t_max = rays["org"], rays["dir"], 100000.0
    n = len(rays)
    assert n % 8 == 0

    def ms(call):
        call()
        return t.stats()["kernelMs"]

    sides = {"query_nearest": lambda: t.query_nearest(org, d, t_max),
             "trace_rays_mode0": lambda: t.trace_rays(0, org, d, t_max),
             "query_any": lambda: t.query_any(org, d, t_max),
             "trace_rays_mode2": lambda: t.trace_rays(2, org, d, t_max),
             "query_nearest_surface": lambda: t.query_nearest(org, d, t_max, surface=True)}
    times = {k: [] for k in sides}
    for rep in range(2 + args.reps):  # two warm-up rounds
        for k, call in sides.items():
            v = ms(call)
            if rep >= 2:
                times[k].append(v)
    hits = t.query_nearest(org, d, t_max)
    same = hits.tobytes() == t.trace_rays(0, org, d, t_max).tobytes()
    occ_same = bool((t.query_any(org, d, t_max) == t.trace_rays(2, org, d, t_max)["t"]).all())
    out = {"workload": "c3_sponza_standin", "size": args.size, "rays": n, "reps": args.reps, "device": t.device_info()[0],
           "compute_units": t.device_info()[1], "source_sha16": prt_amd.test_lib().prt_hip_source_sha16().decode(),
           "hit_fraction": float((hits["t"] != -1).mean()), "answers_equal": {"nearest": same, "any": occ_same},
           "kernel_ms": {k: spread(v) for k, v in times.items()}}
    med = {k: out["kernel_ms"][k]["median"] for k in sides}
    out["query_nearest_over_mode0"] = med["query_nearest"] / med["trace_rays_mode0"]
    out["query_any_over_mode2"] = med["query_any"] / med["trace_rays_mode2"]
    out["surface_over_plain"] = med["query_nearest_surface"] / med["query_nearest"]
    out["mrays_per_s"] = {k: n / med[k] / 1e3 for k in sides}
    t.close()
    emit(out, args.out)


if __name__ == "__main__":
    main()
