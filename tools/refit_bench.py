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

--device measures the device-pointer path instead (include/prt_hip.h "geometry updates from device memory"), every vertex moved:
  (a) prt_hip_deform_meshes with device pointers, PRT_HIP_NORMALS_RECOMPUTE and PRT_HIP_DEFORM_RADIUS_AUTO: wall time of the call,
      the first call apart (it builds the incidence list), and per-kernel HIP-event times (prt_hip_test_deform_profile);
  (b) what it replaces for a caller whose positions are on the device: the device-to-host copy of the positions, the host's
      calculate_vertex_normals, Scene.update_positions (the host refit) and prt_hip_update_meshes, each timed on its own;
and, on the atrium, a series of bend amplitudes: sahCost / sahCostAtUpload of the refitted tree (prt_hip_mesh_info) and the frame
time of the refitted tree against a rebuild (prt_hip_build_bvh) and upload of the same positions and normals.  Writes a text file.

    python tools/refit_bench.py --device [--reps 7] [--scenes c3,c4] [--out profiles/r22_device_deform.txt]
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


def bend_by(P, amplitude):
    return np.ascontiguousarray(P + np.float32(amplitude) * np.sin(np.float32(6.0) * P[:, [1, 2, 0]], dtype=np.float32), dtype=np.float32)


def fmt(v):
    s = spread(v)
    return f"{s['median']:.3f} ({s['min']:.3f}-{s['max']:.3f})"


def frame_ms(t, reps, spp):
    v = []
    for _ in range(reps + 1):
        t.render(spp)
        v.append(t.last_stats["kernelMs"])
    return v[1:]


def upload_rebuilt(t, scene, nodes, remap, P, N, radius):
    """prt_hip_upload_scene of the scene's descriptor with mesh 0's tree, positions and normals replaced"""
    d = scene.describe().contents
    md = prt_amd.MeshDesc.from_buffer_copy(d.meshes[0])
    md.nodeCount, md.nodes = len(nodes), nodes.ctypes.data_as(C.POINTER(prt_amd.BvhNode))
    md.primRemapping = remap.ctypes.data_as(C.POINTER(C.c_uint32))
    md.positions, md.normals = P.ctypes.data_as(C.POINTER(C.c_float)), N.ctypes.data_as(C.POINTER(C.c_float))
    sd = prt_amd.SceneDesc.from_buffer_copy(d)
    sd.meshes, sd.radius = C.pointer(md), radius
    t._chk(t._L.prt_hip_upload_scene(t._ctx, C.byref(sd)), "prt_hip_upload_scene")
    t._scene = scene


def device_mode(args):
    RECOMPUTE = prt_amd.MeshDeform.NORMALS_RECOMPUTE
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("tools/refit_bench.py --device: geometry updates from device memory, every vertex moved")
    for key in args.scenes.split(","):
        name, kw = SCENES[key]
        scene, camera, _ = prt_amd.setup_atrium_standin(960, 540, **kw)
        t = prt_amd.PathTracer(test_entry_points=True)
        if not lines[1:]:
            say(f"source_sha16 {prt_amd.test_lib().prt_hip_source_sha16().decode()}  device {t.device_info()[0]}  reps {args.reps} "
                "(wall times: median (min-max) of the timed calls after warm-up; kernel times: HIP events, median)")
        mesh = scene.arrays()["meshes"][0]
        P0, idx = mesh["positions"], mesh["indices"]
        valence = np.bincount(idx.reshape(-1), minlength=len(P0))
        say()
        say(f"== {key} {name}: {len(idx)} triangles, {len(P0)} vertices; valence mean {valence.mean():.2f}, max {valence.max()}, "
            f"{int((valence > 64).sum())} vertices above 64")
        t.upload_scene(scene)
        t.set_camera(camera)
        P = np.ascontiguousarray(bend(P0))
        with prt_amd.DeviceArrays() as dev:
            dP = dev.upload(P)
            t0 = time.perf_counter()
            t.deform_meshes([(0, dP, RECOMPUTE)])
            first = (time.perf_counter() - t0) * 1e3
            deform = wall_ms(lambda: t.deform_meshes([(0, dP, RECOMPUTE)]), args.reps, 2)
            ups, _ = t._deforms([(0, dP, RECOMPUTE)], False)
            ms = (C.c_float * 5)()
            t._chk(t._L.prt_hip_test_deform_profile(t._ctx, 1, ups, prt_amd.MeshDeform.RADIUS_AUTO, args.reps, ms), "prt_hip_test_deform_profile")
            say(f"(a) prt_hip_deform_meshes, device pointers, RECOMPUTE + RADIUS_AUTO: {fmt(deform)} ms; first call (builds the incidence list) {first:.1f} ms")
            say(f"    kernels: keep + box {ms[0]:.4f}  face normals {ms[1]:.4f}  vertex normals {ms[2]:.4f}  gather {ms[3]:.4f}  levels + finish {ms[4]:.4f}  "
                f"sum {sum(ms):.4f} ms")
            gotP, gotN = t.mesh_vertices(0)
            # (b) the round trip through the host
            back = np.zeros_like(P)
            d2h = wall_ms(lambda: dev.download(back, dP), args.reps, 1)
            one = np.zeros((), dtype=prt_amd.MATERIAL_DTYPE)
            normals = []
            for _ in range(max(3, args.reps // 2)):
                pm = prt_amd.Mesh.from_arrays(idx, back, np.zeros(len(idx), np.uint32), one.reshape(1))
                t0 = time.perf_counter()
                pm.calculate_vertex_normals()
                normals.append((time.perf_counter() - t0) * 1e3)
                del pm
            host_update = wall_ms(lambda: scene.update_positions(0, back, gotN), max(3, args.reps // 2), 1)
            update = wall_ms(lambda: t.update_meshes(scene), args.reps, 2)
            total = sum(float(np.median(v)) for v in (d2h, normals, host_update, update))
            say(f"(b) the host round trip it replaces: device->host copy {fmt(d2h)} + calculate_vertex_normals {fmt(normals)} + "
                f"Scene.update_positions {fmt(host_update)} + prt_hip_update_meshes (positions and normals) {fmt(update)} = {total:.3f} ms")
            say(f"    (b) / (a) = {total / float(np.median(deform)):.1f}")
            a = scene.arrays()
            same = t.mesh_vertices(0)
            say(f"    state check: positions held by the library equal the caller's {same[0].tobytes() == P.tobytes()}; radius {t.mesh_info(0)['radius']!r}, "
                f"host Scene's {a['radius']!r}")
            if key == "c3":
                say()
                say(f"-- bend amplitudes on {key}: P + A sin(6 P.yzx); frame = 960x540, {args.spp} spp, kernel ms median (min-max) of {args.reps}; "
                    "rebuild = prt_hip_build_bvh + prt_hip_upload_scene of the same positions and normals")
                say("   A      sahCost/sahCostAtUpload   refit frame ms            rebuild sahCost ratio   rebuild frame ms          refit / rebuild")
                t.upload_scene(scene_fresh(kw))
                t.set_camera(camera)
                t2 = prt_amd.PathTracer(test_entry_points=True)
                for A in args.amplitudes:
                    PA = bend_by(P0, A)
                    dev.upload(PA, dP)  # (bend_by returns a C-contiguous float32 array of P's size)
                    t.deform_meshes([(0, dP, RECOMPUTE)])
                    info = t.mesh_info(0)
                    refit = frame_ms(t, args.reps, args.spp)
                    _, NA = t.mesh_vertices(0)
                    nodes, remap, _ = t2.build_bvh(idx, PA)
                    upload_rebuilt(t2, scene, nodes, remap, PA, NA, float(info["radius"]))
                    t2.set_camera(camera)
                    info2 = t2.mesh_info(0)
                    rebuilt = frame_ms(t2, args.reps, args.spp)
                    say(f"   {A:<6g} {info['sahCost'] / info['sahCostAtUpload']:<25.4f} {fmt(refit):<25} {info2['sahCost'] / info['sahCostAtUpload']:<23.4f} "
                        f"{fmt(rebuilt):<25} {np.median(refit) / np.median(rebuilt):.3f}")
                t2.close()
        t.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def scene_fresh(kw):
    return prt_amd.setup_atrium_standin(960, 540, **kw)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenes", default="c3,c4")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", action="store_true", help="measure prt_hip_deform_meshes against the host round trip (text output)")
    ap.add_argument("--spp", type=int, default=8, help="--device: samples per pixel of the frames of the amplitude series")
    ap.add_argument("--amplitudes", type=lambda s: [float(x) for x in s.split(",")], default=[0.0, 0.05, 0.2, 0.5, 1.0, 2.0, 4.0])
    args = ap.parse_args()
    prt_amd.build()
    if args.device:
        args.out = args.out or "profiles/r22_device_deform.txt"
        return device_mode(args)
    args.out = args.out or "profiles/r09_refit.json"
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
