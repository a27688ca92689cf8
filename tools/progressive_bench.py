"""Cost of progressive rendering on C3 (BASELINE config 3 stand-in: 1920x1080, depth 8): the same 64 samples per pixel as one
prt_hip_render launch, as 8 accumulate passes of 8 spp and as one accumulate pass of 64 spp.  Times are the library's HIP events
around each frame-kernel launch (kernelMsSum of prt_hip_get_stats, as bench.py reads them) and the host's wall clock over the
frame (launches, the per-launch memsets and events included).  Every variant's image is checked to equal the one-shot image bit
for bit.  Prints one JSON line.

    python tools/progressive_bench.py [--reps 3] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prt_amd  # noqa: E402

W, H, SPP, DEPTH = 1920, 1080, 64, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    prt_amd.build()
    scene, camera, exposure = prt_amd.setup_atrium_standin(W, H, tris=262000, seed=1)
    t = prt_amd.PathTracer()
    t.upload_scene(scene)
    t.set_camera(camera)

    def one_shot():
        t.render_async(0, 0, W - 1, H - 1, SPP, max_depth=DEPTH, exposure=exposure)

    def passes(step):
        def run():
            t.accum_reset()
            for _ in range(SPP // step):
                t.accumulate_async(step, max_depth=DEPTH, exposure=exposure)
        return run

    variants = {"one_shot_64": one_shot, "accumulate_8x8": passes(8), "accumulate_1x64": passes(64)}
    out = {"workload": "c3_sponza_standin", "width": W, "height": H, "spp": SPP, "max_depth": DEPTH, "reps": args.reps,
           "source_sha16": prt_amd.loaded_source_sha16(), "device": t.device_info()[0]}
    ref = None
    for name, run in variants.items():
        for _ in range(args.warmup):
            run()
        t.stats()
        kernel, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            run()
            st = t.stats()  # waits for the frame's launches
            wall.append((time.perf_counter() - t0) * 1e3)
            kernel.append(st["kernelMsSum"])
        img = np.zeros((H, W, 3), dtype=np.float32)
        t._download(img, 0, 0, W - 1, H - 1)
        if ref is None:
            ref = img
        out[name] = {"launches": st["kernelLaunches"], "kernel_ms": float(np.median(kernel)), "wall_ms": float(np.median(wall)),
                     "kernel_ms_all": [round(k, 3) for k in kernel], "wall_ms_all": [round(w, 3) for w in wall],
                     "image_equals_one_shot": bool(img.tobytes() == ref.tobytes())}
    base = out["one_shot_64"]
    for name in ("accumulate_8x8", "accumulate_1x64"):
        v = out[name]
        v["kernel_overhead_frac"] = v["kernel_ms"] / base["kernel_ms"] - 1.0
        v["wall_overhead_frac"] = v["wall_ms"] / base["wall_ms"] - 1.0
    t.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
