"""The denoiser on C3 (BASELINE config 3 stand-in, depth 8) at 1920x1080 and 3840x2160: the prepare kernel, every a-trous iteration by
step and the whole 5-iteration filter, against a plain copy kernel that moves the same compulsory bytes (the yardstick), and against
the 8-spp pass the filter follows.  Times are HIP events inside the TEST build of the library (prt_hip_test_denoise_profile,
prt_hip_test_copy_yardstick: include/prt_hip_test.h): after warm-up calls, `reps` repetitions, median and spread (min, max).  Two states
per size: after ONE 8-spp adaptive pass (one packet per pixel: every variance unknown, no luminance weight is computed) and after TWO
(variances known: the full arithmetic).  The guides' cost (2K G-buffer launches plus their sums) is the wall time of the first
denoise_guides call.  Writes one JSON file stamped with source_sha16 and prints it.

    python tools/denoise_bench.py [--reps 7] [--sizes 1920x1080,3840x2160] [--out profiles/r07_denoise.json]
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

DEPTH, ITERATIONS = 8, 5
# compulsory traffic per pixel as (16-byte planes read, 12-byte planes read, 16-byte planes written, 12-byte planes written)
YARDSTICKS = {"prepare": (2, 2, 3, 0),     # accumulator, moments; albedo, normal -> {C, V}, {A, valid}, {N}
              "iteration": (3, 0, 1, 0),   # {C, V}, {A, valid}, {N} -> {C', V'}
              "last": (3, 0, 1, 1)}        # ... and the image


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default="profiles/r07_denoise.json")
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
        p = t.denoise_params(iterations=ITERATIONS)
        for passes, label in ((1, "after_one_8spp_pass_variance_unknown"), (2, "after_two_8spp_passes_variance_known")):
            t.adaptive_pass_async(8, 0.0, 8 * passes, 8 * passes, exposure=E)
            pass_ms = t.stats()["kernelMs"]
            st = {"pass_8spp_kernel_ms": pass_ms}
            if passes == 1:
                t0 = time.perf_counter()
                t.denoise_guides(p.guideSamples)
                row["guides_first_call_wall_ms"] = (time.perf_counter() - t0) * 1e3
            ms = (C.c_float * 7)()
            runs = []
            for k in range(2 + args.reps):  # two warm-up calls
                t._chk(L.prt_hip_test_denoise_profile(t._ctx, C.byref(p), E, ms), "prt_hip_test_denoise_profile")
                if k >= 2:
                    runs.append(list(ms))
            runs = np.array(runs)
            st["prepare_ms"] = spread(runs[:, 0])
            st["prepare_over_yardstick"] = st["prepare_ms"]["median"] / row["yardstick_ms"]["prepare"]["median"]
            st["iterations"] = []
            for i in range(ITERATIONS):
                kind = "last" if i == ITERATIONS - 1 else "iteration"
                s = dict(spread(runs[:, 1 + i]), step=1 << i, yardstick=kind)
                s["over_yardstick"] = s["median"] / row["yardstick_ms"][kind]["median"]
                st["iterations"].append(s)
            st["whole_denoise_ms"] = spread(runs[:, 6])
            st["denoise_share_of_8spp_pass"] = st["whole_denoise_ms"]["median"] / pass_ms
            row[label] = st
        out["sizes"][size] = row
        t.close()
    text = json.dumps(out, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
