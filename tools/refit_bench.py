"""Moving every vertex of a scene: a new prt_hip_upload_scene against prt_hip_update_meshes, on the C3-class atrium (about 262 k
triangles) and the C4-class scene (2.5 M), one mesh each, vertex normals kept, bump records present.  Per scene, on the same
machine in the same run:
  (a) upload_ms   wall time of prt_hip_upload_scene of the ALREADY BUILT, already host-refitted scene -- what a host has to do per
                  edit without prt_hip_update_meshes (the host refit itself, Scene.update_positions, is not in it);
  (b) update_ms   wall time of prt_hip_update_meshes of all vertices, the copy of the host's arrays and the call's one
                  synchronisation included; gather_ms / levels_ms: HIP-event times of the gather kernel and of the level launches
                  with the finish kernel (prt_hip_test_refit_profile, median of `reps` repetitions inside the library);
  (c) the bytes the two kernels have to read and write, and their times over the copy yardstick of tools/denoise_bench.py
                  (prt_hip_test_copy_yardstick) moving the same number of bytes, half read and half written, as coalesced 16-byte
                  accesses.
Wall times are medians of `reps` timed calls after warm-up calls.  Writes one JSON file stamped with source_sha16 and prints it.

    python tools/refit_bench.py [--reps 7] [--scenes c3,c4] [--out profiles/r09_refit.json]
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

SCENES = {"c3": ("c3_sponza_standin", dict(tris=262000, seed=1)), "c4": ("c4_sanmiguel_standin", dict(tris=2500000, seed=4))}


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def bend(P):
    return (P + np.float32(0.05) * np.sin(np.float32(6.0) * P[:, [1, 2, 0]], dtype=np.float32)).astype(np.float32)


def wall_ms(fn, reps, warm):
    v = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if k >= warm:
            v.append((time.perf_counter() - t0) * 1e3)
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenes", default="c3,c4")
    ap.add_argument("--out", default="profiles/r09_refit.json")
    args = ap.parse_args()
    prt_amd.build()
    out = {"reps": args.reps, "scenes": {}}
    for key in args.scenes.split(","):
        name, kw = SCENES[key]
        scene, camera, _ = prt_amd.setup_atrium_standin(64, 36, **kw)
        t = prt_amd.PathTracer(test_entry_points=True)
        out["source_sha16"], out["device"] = prt_amd.test_lib().prt_hip_source_sha16().decode(), t.device_info()[0]
        mesh = scene.arrays()["meshes"][0]
        scene.update_positions(0, bend(mesh["positions"]))  # the host refit: not timed
        upload = wall_ms(lambda: t.upload_scene(scene), max(3, args.reps // 2), 1)
        t.set_camera(camera)
        update = wall_ms(lambda: t.update_meshes(scene, keep_normals=True), args.reps, 2)
        counts = (C.c_uint64 * 5)()
        t._chk(t._L.prt_hip_test_scene_arrays(t._ctx, counts, None, None, None, None, None, None, None), "prt_hip_test_scene_arrays")
        records, slots, bump = int(counts[0]), int(counts[2]), int(counts[3]) > 0
        prims, verts = len(mesh["indices"]), len(mesh["positions"])
        d = scene.describe().contents
        up = prt_amd.MeshUpdate(0, d.meshes[0].vertexCount, d.meshes[0].positions, None, d.radius)
        ms = (C.c_float * 2)()
        t._chk(t._L.prt_hip_test_refit_profile(t._ctx, 1, C.byref(up), args.reps, ms), "prt_hip_test_refit_profile")
        # what the kernels have to move: ids, the three positions a slot fetches, the triangle, the bump tangents; per record its list
        # entry and kid words, the triangles below its leaf children, the 48-byte box part of its internal children, its own 48 bytes
        gather_bytes = slots * (12 + 36 + 36 + (24 if bump else 0))
        level_bytes = records * (4 + 8 + 48) + 48 * max(records - 1, 0) + 36 * prims
        row = {"workload": name, "triangles": prims, "vertices": verts, "triangle_slots": slots, "node_records": records,
               "upload_ms": spread(upload), "update_ms": spread(update), "update_over_upload": float(np.median(update) / np.median(upload)),
               "host_copy_bytes": 12 * verts, "gather_ms": float(ms[0]), "levels_ms": float(ms[1]), "levels": None,
               "gather_bytes": gather_bytes, "level_bytes": level_bytes}
        for kind, nbytes, kernel_ms in (("gather", gather_bytes, ms[0]), ("levels", level_bytes, ms[1])):
            y, v = C.c_float(), []
            for _ in range(args.reps):
                t._chk(t._L.prt_hip_test_copy_yardstick(t._ctx, (nbytes + 95) // 96, 3, 0, 3, 0, C.byref(y)), "prt_hip_test_copy_yardstick")
                v.append(y.value)
            row[f"{kind}_yardstick_ms"] = spread(v)
            row[f"{kind}_over_yardstick"] = float(kernel_ms / np.median(v))
            row[f"{kind}_GBps"] = float(nbytes / (kernel_ms * 1e-3) / 1e9)
        # depth of the tree = level launches of one update
        second, count = mesh["nodes"]["primOrSecondNodeIndex"].tolist(), mesh["nodes"]["primCount"].tolist()
        depth, deepest = [0] * len(count), -1
        for i in range(len(count)):  # parents come first in depth-first order
            if count[i] == 0xF:
                depth[i + 1] = depth[second[i]] = depth[i] + 1
                deepest = max(deepest, depth[i])
        row["levels"] = deepest + 1
        out["scenes"][key] = row
        t.close()
    text = json.dumps(out, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
