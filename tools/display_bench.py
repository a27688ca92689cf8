"""The display transform on the C3 camera (BASELINE config 3 stand-in, 1920 x 1080, an 8-spp frame): HIP-event medians of its three
kernels (prt_hip_test_display_profile) next to a plain copy kernel that moves the transform's bytes (prt_hip_test_copy_yardstick:
include/prt_hip_test.h), the wall clock of a whole display call with its download, and the path to 8-bit pixels a host had before:
prt_hip_download of the float frame plus the conversion loop of Image::savePpm on one host thread (prt_amd.save_ppm into the null
device).  Diagnostic; prints one line per row.

    python tools/display_bench.py [--reps 9] [--size 1920x1080]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prt_amd  # noqa: E402

YARDSTICK = (1, 2, 0, 1)  # planes read (16 B, 12 B) and written (16 B, 12 B) per element: 52 bytes, 77 % of them read, as the transform's 12 in / 3-4 out


def row(name, v, extra=""):
    v = np.asarray(v, dtype=np.float64)
    print(f"{name:<52} median {np.median(v):9.4f} ms  min {v.min():9.4f}  max {v.max():9.4f}{extra}")
    return float(np.median(v))


def wall(fn, reps):
    out = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]  # the first call warms up


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--size", default="1920x1080")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    prt_amd.build()
    scene, camera, E = prt_amd.setup_atrium_standin(W, H, tris=262000, seed=1)
    t = prt_amd.PathTracer(max_depth=8, test_entry_points=True)
    t.upload_scene(scene)
    t.set_camera(camera)
    L, n = t._L, W * H
    print(f"{a.size}, {n} pixels, {t.device_info()[0]}, library {L.prt_hip_source_sha16().decode()}, reps {a.reps}")
    t.accumulate_async(8, exposure=E)
    print(f"8-spp accumulate pass of the view: kernel {t.stats()['kernelMs']:.3f} ms")
    ms3 = (C.c_float * 3)()
    for name, p in (("RGB8, reference transfer, metered", prt_amd.DisplayParams.make(format=0, transfer=0, meter=True, adapt_rate=0.25)),
                    ("BGRA8, sRGB, metered", prt_amd.DisplayParams.make(format=2, transfer=1, meter=True, adapt_rate=0.25)),
                    ("RGB8, reference transfer, gain 1 (savePpm's bytes)", prt_amd.DisplayParams.make(format=0, transfer=0))):
        print(f"-- {name}")
        v = []
        for _ in range(3):
            t._chk(L.prt_hip_test_display_profile(t._ctx, C.byref(p), a.reps, ms3), "prt_hip_test_display_profile")
            v.append(list(ms3))
        v = np.array(v)
        transform = row("transform kernel (3 medians of reps)", v[:, 2])
        if p.meter:
            row("histogram kernel + memset", v[:, 0])
            row("resolve kernel", v[:, 1])
        nbytes = n * (12 + p.bpp)
        elements = (nbytes + 51) // 52
        y, ms = [], C.c_float()
        for _ in range(a.reps):
            t._chk(L.prt_hip_test_copy_yardstick(t._ctx, elements, *YARDSTICK, C.byref(ms)), "prt_hip_test_copy_yardstick")
            y.append(ms.value)
        copy = row(f"copy yardstick, {nbytes} bytes", y)
        print(f"   transform / yardstick = {transform / copy:.2f}; transform moves {nbytes / transform / 1e6:.0f} GB/s")
        out = np.zeros((H, W, p.bpp), np.uint8)
        t.display_async(p)
        row("prt_hip_download_display (wall, whole image)", wall(lambda: t._chk(L.prt_hip_download_display(t._ctx, out.ctypes.data_as(C.c_void_p), 0, 0, W - 1, H - 1), "download"), a.reps))
        row("display + download_display (wall)", wall(lambda: t.display(p), a.reps))
    print("-- the path without the display transform")
    img = np.zeros((H, W, 3), np.float32)
    down = row("prt_hip_download of the float frame (wall)", wall(lambda: t._download(img, 0, 0, W - 1, H - 1), a.reps))
    sys.stdout.flush()
    null = os.open(os.devnull, os.O_WRONLY)  # savePpm announces every file on stdout
    keep = os.dup(1)
    os.dup2(null, 1)
    try:
        conv = wall(lambda: prt_amd.save_ppm(os.devnull, img, tonemap=True), a.reps)
    finally:
        os.dup2(keep, 1)
        os.close(null)
        os.close(keep)
    conv = row("savePpm's conversion loop, one host thread (wall)", conv)
    got = t.display(prt_amd.DisplayParams.make(format=0, transfer=0))
    host, _ = prt_amd.display_host(img, prt_amd.DisplayParams.make(format=0, transfer=0))
    print(f"download + conversion = {down + conv:.2f} ms; the device's bytes equal the host's: {bool(np.array_equal(got, host))}")


if __name__ == "__main__":
    main()
