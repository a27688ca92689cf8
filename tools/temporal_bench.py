"""The temporal stage on C3 (BASELINE config 3 stand-in, depth 8) at 1920x1080 and 3840x2160: the merge kernel next to the prepare
kernel it replaces, next to one a-trous iteration and next to a plain copy kernel that moves its compulsory bytes (the yardstick);
the whole temporal denoise over the whole plain denoise; and the position pass next to one G-buffer launch of the same view.  Times
are HIP events inside the TEST build of the library (prt_hip_test_temporal_profile, prt_hip_test_denoise_profile,
prt_hip_test_copy_yardstick: include/prt_hip_test.h): after two warm-up calls, `reps` repetitions, median and spread (min, max).
State: view A gets two 8-spp adaptive passes and a temporal denoise, the camera moves sideways, view B gets one 8-spp pass -- the
preview loop's first frame after a move, with the history in place.  Writes one JSON file stamped with source_sha16 and prints it.

    python tools/temporal_bench.py [--reps 7] [--sizes 1920x1080,3840x2160] [--out profiles/r08_temporal.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prt_amd  # noqa: E402

DEPTH, ITERATIONS = 8, 5
# compulsory traffic per pixel as (16-byte planes read, 12-byte planes read, 16-byte planes written, 12-byte planes written)
YARDSTICKS = {"merge": (6, 2, 6, 0),     # accumulator, moments, position, three history planes; albedo, normal -> three filter planes, pending
              "prepare": (2, 2, 3, 0),
              "iteration": (3, 0, 1, 0)}


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default="profiles/r08_temporal.json")
    args = ap.parse_args()
    prt_amd.build()
    out = {"workload": "c3_sponza_standin", "max_depth": DEPTH, "reps": args.reps, "iterations": ITERATIONS, "sizes": {}}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        scene, camera, E = prt_amd.setup_atrium_standin(W, H, tris=262000, seed=1)
        t = prt_amd.PathTracer(max_depth=DEPTH, test_entry_points=True)
        t.upload_scene(scene)
        t.set_camera(camera)
        out["source_sha16"], out["device"] = prt_amd.test_lib().prt_hip_source_sha16().decode(), t.device_info()[0]
        L, n = t._L, W * H
        row = {"pixels": n}

        def copy_ms(kind):
            ms = C.c_float()
            v = []
            for _ in range(args.reps):
                t._chk(L.prt_hip_test_copy_yardstick(t._ctx, n, *YARDSTICKS[kind], C.byref(ms)), "prt_hip_test_copy_yardstick")
                v.append(ms.value)
            r16, r12, w16, w12 = YARDSTICKS[kind]
            return dict(spread(v), bytes_per_pixel=16 * (r16 + w16) + 12 * (r12 + w12))

        row["yardstick_ms"] = {k: copy_ms(k) for k in YARDSTICKS}
        for passes in (1, 2):
            t.adaptive_pass_async(8, 0.0, 8 * passes, 8 * passes, exposure=E)
        t.stats()
        t.denoise_temporal_async(exposure=E)
        # the same scene from a little to the side: the scene's radius scales the step
        box = scene.bbox()
        shift = 0.01 * float(np.linalg.norm(box[3:] - box[:3]))
        moved = prt_amd.Camera().create(tuple(float(v) for v in camera.pos_arg + np.array([shift, 0.0, 0.0], np.float32)),
                                        tuple(float(v) for v in camera.dir_arg), W, H)
        t.set_camera(moved)
        t.adaptive_pass_async(8, 0.0, 8, 8, exposure=E)
        row["pass_8spp_kernel_ms"] = t.stats()["kernelMs"]
        p, tp = t.denoise_params(iterations=ITERATIONS), t.temporal_params()
        t.denoise_temporal_async(exposure=E)
        pend = t.history_export(1)
        hit = t.denoise_position()[..., 3] >= 0
        row["hit_pixels"] = int(hit.sum())
        row["pixels_with_history"] = int((hit & (pend["pos_len"][..., 3] > 8)).sum())
        ms4, ms7 = (C.c_float * 4)(), (C.c_float * 7)()
        temporal, plain = [], []
        for k in range(2 + args.reps):  # two warm-up calls
            t._chk(L.prt_hip_test_temporal_profile(t._ctx, C.byref(p), C.byref(tp), E, ms4), "prt_hip_test_temporal_profile")
            t._chk(L.prt_hip_test_denoise_profile(t._ctx, C.byref(p), E, ms7), "prt_hip_test_denoise_profile")
            if k >= 2:
                temporal.append(list(ms4))
                plain.append(list(ms7))
        temporal, plain = np.array(temporal), np.array(plain)
        row["merge_ms"] = spread(temporal[:, 0])
        row["prepare_ms"] = spread(plain[:, 0])
        row["iteration_ms"] = [dict(spread(plain[:, 1 + i]), step=1 << i) for i in range(ITERATIONS)]
        row["merge_over_yardstick"] = row["merge_ms"]["median"] / row["yardstick_ms"]["merge"]["median"]
        row["merge_over_prepare"] = row["merge_ms"]["median"] / row["prepare_ms"]["median"]
        row["merge_over_first_iteration"] = row["merge_ms"]["median"] / row["iteration_ms"][0]["median"]
        row["whole_temporal_denoise_ms"] = spread(temporal[:, 1])
        row["whole_plain_denoise_ms"] = spread(plain[:, 6])
        row["temporal_over_plain"] = row["whole_temporal_denoise_ms"]["median"] / row["whole_plain_denoise_ms"]["median"]
        row["position_pass_ms"] = spread(temporal[:, 2])
        row["gbuffer_launch_ms"] = spread(temporal[:, 3])
        row["position_over_gbuffer"] = row["position_pass_ms"]["median"] / row["gbuffer_launch_ms"]["median"]
        out["sizes"][size] = row
        t.close()
    text = json.dumps(out, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
