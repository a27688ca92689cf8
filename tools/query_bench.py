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
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prt_amd  # noqa: E402


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    prt_amd.build()
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
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
