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

--bake: prt_hip_bake (include/prt_hip.h "baking").  4096 and 65 536 points (first hits of the same camera's rays) with one cosine set of
K = 64 and K = 256 directions, 8 spp, depth 8: (a) one prt_hip_bake on device arrays, (b) rays in numpy, query_radiance on host arrays
and a numpy mean, (c) the frame-kernel launch inside (a); and the two new kernels alone.  The ratio to read is (a) / (c).

    python tools/query_bench.py --bake [--reps 5] [--out F]

--atlas: the lightmap atlas calls (include/prt_hip.h "lightmap atlases").  Every triangle of the scene gets a cell of its own in a grid,
into a 1024 x 1024 and a 4096 x 4096 atlas; one cosine set of K = 16 directions, 8 spp, depth 8, gutter 2: each of the three new calls
alone on device arrays, lightmap() end to end against the frame-kernel launches inside it, and ONE run of the route it replaces: the
numpy rasteriser, points and gutter fill of tests/prt_atlas_ref.py around bake() on host arrays.

    python tools/query_bench.py --atlas [--reps 5] [--out F]

--lens: prt_hip_lens_render (include/prt_hip.h "lens renders") from the bench camera's position, 8 spp, depth 8: a 2048 x 1024 panorama
with K = 1, a 1920 x 1080 thin-lens pinhole with K = 8 (16.6 M rays, one band) and the same at 3840 x 2160 (four bands).  Per workload:
(a) one call on device memory, (c) the sum of the frame-kernel launches inside it, the two new kernels alone on one band, and (b) the
route it replaces: rays in numpy, query_radiance on host arrays in chunks the caller cuts, numpy sums.  The ratio to read is (a) / (c).
Also the accumulate kernel alone over 2^24 radiances at K = 1, 8 and 64: the layout of its reads is the one thing K changes.

    python tools/query_bench.py --lens [--reps 3] [--out F]

--atlas-filter: prt_hip_atlas_filter (include/prt_hip.h "lightmap filter") on the atlases of --atlas (one grid cell per triangle, 1024 x
1024 and 4096 x 4096), K = 16 directions, 8 spp, C = 1, five iterations at the default parameters: per kernel (HIP events inside the TEST
build's prt_hip_test_atlas_filter_profile) and the whole call on device arrays, against the bake launches of the same points, per point
and iteration, and against ONE run of the numpy restatement tests/prt_atlas_filter_ref.py; and the RMSE of the 8-spp values, unfiltered
and filtered, against a bake of the same points at --ref-spp (1024 x 1024 only, and on the Cornell box in a 256 x 256 atlas, whose 36
triangles make charts of some 500 texels where the stand-in's are a few texels each).

    python tools/query_bench.py --atlas-filter [--reps 5] [--ref-spp 2040] [--out F]

--visibility: prt_hip_bake_visibility (include/prt_hip.h "visibility baking") on the 1024 x 1024 atlas of --atlas (one grid cell per
triangle), one cosine set of K = 64 directions with weights 1/K, maxDistance +inf and a tenth of the scene's radius.  (a) the call
end to end on device arrays (host clock between synchronisations), its trace kernel (event pair, prt_hip_get_stats) and its reduce
alone (prt_hip_bake_visibility_reduce on the bytes, host clock); (b) prt_hip_query_any alone on the same rays, materialised once in
parts of 2^24 rays by prt_hip_bake_rays with tMax written on the host: the traversal floor, on code the visibility baker does not
touch; (c) the bake_rays kernel for the same rays (host clock); (d) ONE run of the host-array route every caller had: bake_rays,
numpy tMax, query_any, numpy sum.  The bytes of (a), (b) and (d) must be equal.

    python tools/query_bench.py --visibility [--reps 5] [--out F]
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


def fetch(dev, p, count, dtype):
    """`count` elements of `dtype` from device address p (the null stream: behind the context's blocking stream)."""
    out = np.zeros(count, dtype=dtype)
    dev.download(out, p)
    return out


def bake(args):
    """Points = the first hits of pixel-centre rays at equal strides over the image (position and shading normal from query_nearest's
    surface records), one cosine set of K directions.  Per (n, K): (a) prt_hip_bake on device arrays, wall time of the call up to
    the synchronisation behind it; (c) the frame-kernel launch inside (a), kernelMs; the two new kernels alone on device arrays
    (prt_hip_bake_rays, prt_hip_bake_reduce: wall time up to the synchronisation); (b) the route there was before: rays built in numpy,
    query_radiance on host arrays, a numpy weighted mean.  The largest difference between the answers of (a) and (b) is reported, not
    asserted: the host's frame is built in double precision, and a direction that differs in its last bit sends some path elsewhere
    (equality byte for byte with the same rays is what tests/test_gpu_bake.py holds)."""
    W, H = (int(v) for v in args.size.split("x"))
    spp, depth, seed = 8, 8, 12345
    scene, camera, _ = prt_amd.setup_atrium_standin(W, H, tris=262000, seed=1)
    t = prt_amd.PathTracer(max_depth=depth, seed=seed)
    t.upload_scene(scene)
    out = {"workload": "c3_sponza_standin", "points_from": args.size + " first hits at equal strides", "spp": spp, "max_depth": depth,
           "reps": args.reps, "device": t.device_info()[0], "compute_units": t.device_info()[1],
           "source_sha16": prt_amd.loaded_source_sha16(), "bake": {}}
    sync = lambda: t.stats()  # noqa: E731  (prt_hip_get_stats synchronises the context's stream)
    for n in (4096, 65536):
        idx = (np.arange(4 * n, dtype=np.uint64) * np.uint64(W * H) // np.uint64(4 * n)).astype(np.uint32)
        ys, xs = np.divmod(idx, np.uint32(W))
        r = prt_amd.pixel_centre_rays(camera.desc, xs, ys)
        hits, surf = t.query_nearest(r["org"], r["dir"], r["tMax"], surface=True)
        surf = surf[hits["t"] != -1][:n]
        assert len(surf) == n, "too few first hits"
        pts = prt_amd.make_bake_points(surf["P"], surf["shadingNormal"], 1e-4)
        for K in (64, 256):
            d, w = prt_amd.bake_cosine_set(K, np.random.default_rng(K))
            with prt_amd.DeviceArrays() as dev:
                d_pts, d_dirs, d_w, d_out, d_rays, d_rad = (dev.upload(a) for a in (pts, d, w, np.zeros(n * 3, np.float32), np.zeros(n * K, prt_amd.RAY_DTYPE),
                                                                                       np.zeros((n * K, 3), np.float32)))
                table = prt_amd.BakeSets(K=K, C=1, nSets=1, reserved=0, dirs=d_dirs, weights=d_w)
                p = t._probe_params(spp, None, None, None)
                times = {k: [] for k in ("a_bake_wall", "c_frame_kernel", "rays_kernel_wall", "reduce_kernel_wall", "b_host_route_wall",
                                         "b_numpy_rays", "b_query_radiance", "b_numpy_reduce")}
                host = None
                for rep in range(2 + args.reps):
                    keep = rep >= 2
                    sync()
                    t0 = time.perf_counter()
                    t.bake_async(n, d_pts, table, d_out, spp)
                    st = t.stats()
                    dt = (time.perf_counter() - t0) * 1e3
                    if keep:
                        times["a_bake_wall"].append(dt)
                        times["c_frame_kernel"].append(st["kernelMs"])
                    for name, call in (("rays_kernel_wall", lambda: t._L.prt_hip_bake_rays(t._ctx, n, d_pts, C.byref(table), d_rays, 0, None)),
                                       ("reduce_kernel_wall", lambda: t._L.prt_hip_bake_reduce(t._ctx, n, d_pts, C.byref(table), d_rad, d_out, 0, None))):
                        sync()
                        t0 = time.perf_counter()
                        assert call() == 0
                        sync()
                        if keep:
                            times[name].append((time.perf_counter() - t0) * 1e3)
                    if rep in (0, 2 + args.reps - 1) or (keep and n * K <= 1 << 20):  # (the host route at 16.8 M rays: once warm, once timed)
                        t0 = time.perf_counter()
                        rays = host_rays(pts, d)
                        t1 = time.perf_counter()
                        L = t.query_radiance(rays["org"], rays["dir"], spp)
                        t2 = time.perf_counter()
                        host = (np.pi * L.reshape(n, K, 3).mean(axis=1, dtype=np.float64)).astype(np.float32)
                        t3 = time.perf_counter()
                        if keep:
                            for k, v in (("b_host_route_wall", t3 - t0), ("b_numpy_rays", t1 - t0), ("b_query_radiance", t2 - t1), ("b_numpy_reduce", t3 - t2)):
                                times[k].append(v * 1e3)
                t.bake_async(n, d_pts, table, d_out, spp)
                rays_traced = t.stats()["raysTraced"]
                got = fetch(dev, d_out, n * 3, np.float32).reshape(n, 3)
            a, c = float(np.median(times["a_bake_wall"])), float(np.median(times["c_frame_kernel"]))
            out["bake"][f"{n}x{K}"] = {
                "ms": {k: spread(v) for k, v in times.items()}, "rays_traced": rays_traced,
                "a_over_c": a / c, "b_over_a": float(np.median(times["b_host_route_wall"])) / a,
                "new_kernels_share_of_a": (float(np.median(times["rays_kernel_wall"])) + float(np.median(times["reduce_kernel_wall"]))) / a,
                "largest_difference_from_host_route": float(np.abs(got - host).max()), "largest_value": float(np.abs(host).max())}
    t.close()
    emit(out, args.out)


def atlas(args):
    """Per atlas size: rasterize, points and resolve alone on device arrays (wall time from a synchronised stream to the
    synchronisation behind the call; rasterize synchronises itself), lightmap() end to end (wall) against kernelMs of the prt_hip_bake
    launches inside it, and the host route once: numpy rasteriser, numpy points with query_surface's normals, bake() on host arrays in
    parts of 2^24 rays, numpy gutter fill.  The host route's image must equal lightmap()'s byte for byte."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import prt_atlas_ref as AR
    spp, depth, seed, K, gutter, bias = 8, 8, 12345, 16, 2, 1e-4
    scene, _, _ = prt_amd.setup_atrium_standin(64, 64, tris=262000, seed=1)
    t = prt_amd.PathTracer(max_depth=depth, seed=seed)
    t.upload_scene(scene)
    meshes = scene.arrays()["meshes"]
    prims = [len(m["indices"]) for m in meshes]
    total = sum(prims)
    G = int(np.ceil(np.sqrt(total)))
    cell = np.arange(total)
    corner = np.array([(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)])
    uv_all = ((np.stack([cell % G, cell // G], axis=1)[:, None, :] + corner[None]) / G).astype(np.float32)
    uvs = {m: uv_all[sum(prims[:m]):sum(prims[:m + 1])] for m in range(len(prims))}
    d, w = prt_amd.bake_cosine_set(K, np.random.default_rng(K))
    out = {"workload": "c3_sponza_standin", "layout": f"{total} triangles of {len(prims)} meshes, one cell each of a {G} x {G} grid", "K": K,
           "spp": spp, "max_depth": depth, "gutter": gutter, "reps": args.reps, "device": t.device_info()[0],
           "compute_units": t.device_info()[1], "source_sha16": prt_amd.loaded_source_sha16(), "atlas": {}}
    sync = lambda: t.stats()  # noqa: E731  (prt_hip_get_stats synchronises the context's stream)
    for W in (1024, 4096):
        H = W
        with prt_amd.DeviceArrays() as dev:
            d_uv = {m: dev.upload(uv) for m, uv in uvs.items()}
            d_texels, d_hits = dev.upload(np.zeros(W * H, np.uint32)), dev.upload(np.zeros(W * H, prt_amd.HIT_DTYPE))
            rasterize = lambda: t.atlas_rasterize_device(W, H, d_uv, dict(enumerate(prims)), d_texels, d_hits)  # noqa: E731
            counts = rasterize()
            n = counts["n"]
            d_points, d_values, d_image, d_mask = (dev.upload(a) for a in (np.zeros(n, prt_amd.BAKE_POINT_DTYPE), np.zeros((n, 3), np.float32),
                                                                           np.zeros((W * H, 3), np.float32), np.zeros(W * H, np.uint8)))
            times = {k: [] for k in ("rasterize_wall", "points_wall", "resolve_wall", "lightmap_wall", "bake_kernels")}
            image = mask = None
            for rep in range(2 + args.reps):
                keep = rep >= 2
                for name, call in (("rasterize_wall", rasterize), ("points_wall", lambda: t.atlas_points_async(n, W, d_texels, d_hits, d_points, bias=bias)),
                                   ("resolve_wall", lambda: t.atlas_resolve_async(W, H, n, d_texels, d_values, 3, gutter, d_image, d_mask))):
                    sync()
                    t0 = time.perf_counter()
                    call()
                    sync()
                    if keep:
                        times[name].append((time.perf_counter() - t0) * 1e3)
                sync()
                t0 = time.perf_counter()
                image, mask = t.lightmap(uvs, W, H, d, w, spp, bias=bias, gutter=gutter)
                dt = (time.perf_counter() - t0) * 1e3
                if keep:
                    times["lightmap_wall"].append(dt)
                    times["bake_kernels"].append(t.last_stats["kernelMsSum"])  # (a bake of more than 2^24 rays is several launches)
            launches, rays_last = t.last_stats["kernelLaunches"], t.last_stats["raysTraced"]
        # the route it replaces, once
        host = {}
        t0 = time.perf_counter()
        texels, hits, host_counts = AR.rasterize(uvs, W, H)
        host["numpy_rasterize"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        zero = np.zeros((len(hits), 3), np.float32)
        pts = AR.points(texels, hits, W, [(m["indices"], m["positions"]) for m in meshes], t.query_surface(zero, zero, hits)["normal"], bias, 1)
        host["numpy_points_with_query_surface"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        part = (1 << 24) // K
        baked = np.concatenate([t.bake(pts["P"][i0:i0 + part], pts["N"][i0:i0 + part], d, w, spp, bias=pts["bias"][i0:i0 + part],
                                       seed=(seed + i0 * K) & 0xffffffff) for i0 in range(0, len(pts), part)])
        host["bake_on_host_arrays"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        host_image, host_mask = AR.resolve(texels, baked.reshape(len(texels), -1), W, H, gutter)
        host["numpy_resolve"] = time.perf_counter() - t0
        med = {k: float(np.median(v)) for k, v in times.items()}
        new_calls = med["rasterize_wall"] + med["points_wall"] + med["resolve_wall"]
        out["atlas"][f"{W}x{H}"] = {
            "counts": counts, "host_counts_equal": host_counts == counts, "bake_launches": launches, "rays_traced_by_the_last_launch": rays_last,
            "ms": {k: spread(v) for k, v in times.items()}, "lightmap_over_bake_kernels": med["lightmap_wall"] / med["bake_kernels"],
            "three_calls_share_of_bake_kernels": new_calls / med["bake_kernels"],
            "host_route_ms": {k: v * 1e3 for k, v in host.items()}, "host_route_total_ms": sum(host.values()) * 1e3,
            "host_route_over_lightmap": sum(host.values()) * 1e3 / med["lightmap_wall"],
            "host_route_without_bake_over_three_calls": (sum(host.values()) - host["bake_on_host_arrays"]) * 1e3 / new_calls,
            "images_equal": image.tobytes() == host_image.tobytes() and mask.tobytes() == host_mask.tobytes(),
            "lit_fraction_of_owned": float((image.reshape(-1, 3)[mask.reshape(-1) == 1] != 0).any(axis=1).mean())}
    t.close()
    emit(out, args.out)


def atlas_filter(args):
    """Per workload: rasterize, points and an 8-spp bake on device arrays; then (a) the filter's whole call (host clock around
    atlas_filter_async up to the synchronisation, and the event pair of the profile entry point), its kernels by events, (b) kernelMsSum
    of the bake launches, (c) the numpy restatement once on host arrays -- whose output must equal the product's byte for byte."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import prt_atlas_filter_ref as AF
    spp, depth, seed, K, bias = 8, 8, 12345, 16, 1e-4
    d, w = prt_amd.bake_cosine_set(K, np.random.default_rng(K))
    params = prt_amd.AtlasFilterParams()
    out = {"K": K, "spp": spp, "max_depth": depth, "reps": args.reps, "ref_spp": args.ref_spp, "source_sha16": prt_amd.loaded_source_sha16(),
           "params": {k: getattr(params, k) for k in ("iterations", "normalPowerLog2", "sigmaLuminance", "sigmaPosition")}, "atlas_filter": {}}
    workloads = [("c3_sponza_standin", lambda: prt_amd.setup_atrium_standin(64, 64, tris=262000, seed=1)[0], 1024, args.ref_spp),
                 ("c3_sponza_standin", None, 4096, 0),
                 ("cornell_box", lambda: prt_amd.setup_cornell_box(64, 64)[0], 256, args.ref_spp)]
    t = None
    for name, make, W, ref_spp in workloads:
        if make is not None:
            if t is not None:
                t.close()
            scene = make()
            t = prt_amd.PathTracer(max_depth=depth, seed=seed, test_entry_points=True)
            t.upload_scene(scene)
            out["device"], out["compute_units"] = t.device_info()[0], t.device_info()[1]
            prims = [len(m["indices"]) for m in scene.arrays()["meshes"]]
            total = sum(prims)
            G = int(np.ceil(np.sqrt(total)))
            cell = np.arange(total)
            corner = np.array([(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)])
            uv_all = ((np.stack([cell % G, cell // G], axis=1)[:, None, :] + corner[None]) / G).astype(np.float32)
            uvs = {m: uv_all[sum(prims[:m]):sum(prims[:m + 1])] for m in range(len(prims))}
        H = W
        sync = lambda: t.stats()  # noqa: E731  (prt_hip_get_stats synchronises the context's stream)
        with prt_amd.DeviceArrays() as dev:
            d_uv = {m: dev.upload(uv) for m, uv in uvs.items()}
            d_texels, d_hits = dev.alloc(4 * W * H), dev.alloc(prt_amd.HIT_DTYPE.itemsize * W * H)
            n = t.atlas_rasterize_device(W, H, d_uv, dict(enumerate(prims)), d_texels, d_hits)["n"]
            d_points, d_values, d_out, d_ref = (dev.alloc(s_ * n) for s_ in (32, 12, 12, 12))
            t.atlas_points_async(n, W, d_texels, d_hits, d_points, bias=bias)
            table = prt_amd.BakeSets(K=K, C=1, nSets=1, reserved=0, dirs=dev.upload(d), weights=dev.upload(w))

            def bake_into(dst, samples):
                ms, part = 0.0, max(1, (1 << 24) // K)
                for i0 in range(0, n, part):
                    t.bake_async(min(part, n - i0), d_points + 32 * i0, table, dst + 12 * i0, samples, seed=(seed + i0 * K) & 0xffffffff)
                    ms += t.stats()["kernelMs"]
                return ms
            times = {k: [] for k in ("bake_kernels", "filter_wall", "filter_events", "index", "prepare", "iter0", "iter1", "iter2", "iter3", "iter4")}
            ms = (C.c_float * 8)()
            for rep in range(1 + args.reps):
                bake_ms = bake_into(d_values, spp)
                sync()
                t0 = time.perf_counter()
                t.atlas_filter_async(W, H, n, d_texels, d_points, d_values, 3, d_out, params)
                sync()
                wall = (time.perf_counter() - t0) * 1e3
                t._chk(t._L.prt_hip_test_atlas_filter_profile(t._ctx, W, H, n, d_texels, d_points, d_values, 3, C.byref(params), d_out, ms),
                       "prt_hip_test_atlas_filter_profile")
                if rep >= 1:
                    for k, v in zip(("index", "prepare", "iter0", "iter1", "iter2", "iter3", "iter4", "filter_events"), ms):
                        times[k].append(float(v))
                    times["bake_kernels"].append(bake_ms)
                    times["filter_wall"].append(wall)
            texels, points = fetch(dev, d_texels, n, np.uint32), fetch(dev, d_points, n, prt_amd.BAKE_POINT_DTYPE)
            values, got = fetch(dev, d_values, 3 * n, np.float32).reshape(n, 3), fetch(dev, d_out, 3 * n, np.float32).reshape(n, 3)
            t0 = time.perf_counter()
            want = AF.filter(texels, points, values, W, H)
            numpy_ms = (time.perf_counter() - t0) * 1e3
            is_placed, _ = AF.placed(texels, points.view(AF.POINT_DTYPE), values, W, H)
            med = {k: float(np.median(v)) for k, v in times.items()}
            iters = [med[f"iter{i}"] for i in range(5)]
            row = {"n": int(n), "placed": int(is_placed.sum()), "ms": {k: spread(v) for k, v in times.items()},
                   "filter_share_of_bake_kernels": med["filter_events"] / med["bake_kernels"],
                   "ns_per_point_and_iteration": [1e6 * v / n for v in iters], "numpy_restatement_ms": numpy_ms,
                   "numpy_over_filter": numpy_ms / med["filter_wall"], "equals_the_restatement": got.tobytes() == want.tobytes(),
                   "changed_fraction": float((got != values).any(axis=1).mean())}
            if ref_spp:
                row["reference_bake_kernels_ms"] = bake_into(d_ref, ref_spp)
                ref = fetch(dev, d_ref, 3 * n, np.float32).reshape(n, 3).astype(np.float64)
                rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - ref) ** 2)))  # noqa: E731  (every point is a texel of mask 1)
                row.update(rmse_unfiltered=rmse(values), rmse_filtered=rmse(got), rmse_ratio=rmse(values) / rmse(got), reference_mean=float(ref.mean()))
            out["atlas_filter"][f"{name} {W}x{H}"] = row
    t.close()
    emit(out, args.out)


def lens_host_band(lens, y0, y1, rng):
    """What a caller wrote in numpy for rows [y0, y1): jittered film coordinates, the model's direction, the
    thin lens's disc, in double precision with a generator of its own: (org, dir) of (y1 - y0) * W * K rays."""
    W, H, K = lens.width, lens.height, lens.K
    pos, fwd, right, up = (np.array(list(getattr(lens, k)), np.float64) for k in ("pos", "fwd", "right", "up"))
    y, x, _ = np.meshgrid(np.arange(y0, y1), np.arange(W), np.arange(K), indexing="ij")
    n = x.size
    a = 2.0 * (x.reshape(-1) + rng.random(n)) / W - 1.0
    b = 1.0 - 2.0 * (y.reshape(-1) + rng.random(n)) / H
    org = np.broadcast_to(pos, (n, 3))
    if lens.model == prt_amd.LENS_EQUIRECT:
        phi, th = a * np.pi, b * (np.pi / 2)
        l = np.stack([np.cos(th) * np.sin(phi), np.sin(th), np.cos(th) * np.cos(phi)], axis=1)
        d = l[:, 0:1] * right + l[:, 1:2] * up + l[:, 2:3] * fwd
    else:
        d = fwd + a[:, None] * right + b[:, None] * up
        if lens.lensRadius > 0:
            rl, phi = lens.lensRadius * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
            R, U = right / np.linalg.norm(right), up / np.linalg.norm(up)
            org = pos + (rl * np.cos(phi))[:, None] * R + (rl * np.sin(phi))[:, None] * U
            d = pos + lens.focus * d - org
    return org, d


def lens(args):
    """Per workload: (a) prt_hip_lens_render on device memory, wall time of the call up to the synchronisation behind it; (c) the
    frame-kernel launches inside (a), kernelMsSum over kernelLaunches; the two new kernels alone on the rows of one band, on device
    arrays (wall time up to the synchronisation); (b) the route there was before, once: lens_host_band, query_radiance on host
    arrays per chunk of at most 2^24 rays, a numpy sum over K.  (b) draws other jitter, so its image is compared by its mean only."""
    spp, depth, seed = 8, 8, 12345
    scene, camera, _ = prt_amd.setup_atrium_standin(1920, 1080, tris=262000, seed=1)
    t = prt_amd.PathTracer(max_depth=depth, seed=seed)
    t.upload_scene(scene)
    out = {"workload": "c3_sponza_standin", "spp": spp, "max_depth": depth, "reps": args.reps, "device": t.device_info()[0],
           "compute_units": t.device_info()[1], "source_sha16": prt_amd.loaded_source_sha16(), "lens": {}, "accumulate_alone": {}}
    c = camera.desc
    pos = np.array(list(c.pos), np.float64)
    at, up = pos + np.array(list(c.dir), np.float64), (0.0, 1.0, 0.0)
    sync = lambda: t.stats()  # noqa: E731  (prt_hip_get_stats synchronises the context's stream)
    with prt_amd.DeviceArrays() as scratch:
        d_rays, d_rad = scratch.upload(np.zeros(1 << 24, prt_amd.RAY_DTYPE)), scratch.upload(np.zeros((1 << 24, 3), np.float32))
        workloads = {"equirect_2048x1024_K1": prt_amd.lens_equirect(pos, 2048, 1024, K=1, fwd=list(c.dir), jitter_seed=1),
                     "thin_lens_1920x1080_K8": prt_amd.lens_pinhole(pos, at, up, 0.9, 1920, 1080, K=8, lens_radius=0.05, focus=6.0, jitter_seed=1),
                     "thin_lens_3840x2160_K8": prt_amd.lens_pinhole(pos, at, up, 0.9, 3840, 2160, K=8, lens_radius=0.05, focus=6.0, jitter_seed=1)}
        for name, d in workloads.items():
            W, H, K = d.width, d.height, d.K
            rows = min(H, (1 << 24) // (W * K))
            with prt_amd.DeviceArrays() as dev:
                image = dev.upload(np.zeros(W * H * 3, np.float32))
                times = {k: [] for k in ("a_lens_render_wall", "c_frame_kernels", "rays_kernel_wall", "accumulate_kernel_wall")}
                launches = 0
                for rep in range(1 + args.reps):  # one warm-up round
                    sync()
                    t0 = time.perf_counter()
                    t.render_lens_async(d, image, spp)
                    st = t.stats()
                    dt = (time.perf_counter() - t0) * 1e3
                    launches = st["kernelLaunches"]
                    if rep:
                        times["a_lens_render_wall"].append(dt)
                        times["c_frame_kernels"].append(st["kernelMsSum"])
                    for key, call in (("rays_kernel_wall", lambda: t._L.prt_hip_lens_rays(t._ctx, C.byref(d), 0, rows, d_rays, 0, None)),
                                      ("accumulate_kernel_wall", lambda: t._L.prt_hip_lens_accumulate(t._ctx, C.byref(d), 0, rows, d_rad, image, 0, None))):
                        sync()
                        t0 = time.perf_counter()
                        assert call() == 0
                        sync()
                        if rep:
                            times[key].append((time.perf_counter() - t0) * 1e3)
                t.render_lens_async(d, image, spp)
                rays_traced_last_band = t.stats()["raysTraced"]
                got = fetch(dev, image, W * H * 3, np.float32).reshape(H, W, 3) / np.float32(K)
            # (b), once: the chunks are the caller's to cut
            rng = np.random.default_rng(7)
            host = np.zeros((H, W, 3), np.float32)
            tb = {"numpy_rays": 0.0, "query_radiance": 0.0, "numpy_sum": 0.0}
            t0 = time.perf_counter()
            for y0 in range(0, H, rows):
                y1 = min(H, y0 + rows)
                t1 = time.perf_counter()
                org, dr = lens_host_band(d, y0, y1, rng)
                t2 = time.perf_counter()
                L = t.query_radiance(org, dr, spp, seed=seed + y0 * W * K)
                t3 = time.perf_counter()
                host[y0:y1] = L.reshape(y1 - y0, W, K, 3).sum(axis=2) / np.float32(K)
                t4 = time.perf_counter()
                tb["numpy_rays"] += (t2 - t1) * 1e3
                tb["query_radiance"] += (t3 - t2) * 1e3
                tb["numpy_sum"] += (t4 - t3) * 1e3
                del org, dr, L
            b_ms = (time.perf_counter() - t0) * 1e3
            a, cc = float(np.median(times["a_lens_render_wall"])), float(np.median(times["c_frame_kernels"]))
            out["lens"][name] = {
                "rays": W * H * K, "bands": launches, "rows_per_band": rows, "ms": {k: spread(v) for k, v in times.items()},
                "a_over_c": a / cc, "b_host_route_wall_ms": b_ms, "b_parts_ms": tb, "b_over_a": b_ms / a,
                "new_kernels_ms_per_call": (float(np.median(times["rays_kernel_wall"])) + float(np.median(times["accumulate_kernel_wall"]))) * launches,
                "rays_traced_last_band": rays_traced_last_band, "image_mean": float(got.mean(dtype=np.float64)),
                "host_route_image_mean": float(host.mean(dtype=np.float64))}
        # the accumulate kernel alone: 2^24 radiances (201 MB read) into 2^24 / K pixels
        for K, (W, H) in ((1, (4096, 4096)), (8, (2048, 1024)), (64, (512, 512))):
            d = prt_amd.lens_pinhole(pos, at, up, 0.9, W, H, K=K)
            with prt_amd.DeviceArrays() as dev:
                image = dev.upload(np.zeros(W * H * 3, np.float32))
                ms = []
                for rep in range(2 + args.reps):
                    sync()
                    t0 = time.perf_counter()
                    assert t._L.prt_hip_lens_accumulate(t._ctx, C.byref(d), 0, H, d_rad, image, 0, None) == 0
                    sync()
                    if rep >= 2:
                        ms.append((time.perf_counter() - t0) * 1e3)
            nbytes = 12 * (1 << 24) + 12 * W * H
            out["accumulate_alone"][f"K{K}"] = {"pixels": W * H, "wall_ms": spread(ms), "GB_per_s": nbytes / float(np.median(ms)) / 1e6}
    t.close()
    emit(out, args.out)


def visibility(args):
    """See the module's docstring.  Every timed call follows two warm-up calls; the sides are interleaved per repetition."""
    K, bias, W = 64, 1e-4, 1024
    scene, _, _ = prt_amd.setup_atrium_standin(64, 64, tris=262000, seed=1)
    t = prt_amd.PathTracer(max_depth=8)
    t.upload_scene(scene)
    L, ctx = t._L, t._ctx
    box = np.array(scene.bbox(), np.float64).reshape(2, 3)
    radius = 0.5 * float(np.linalg.norm(box[1] - box[0]))
    meshes = scene.arrays()["meshes"]
    prims = [len(m["indices"]) for m in meshes]
    total = sum(prims)
    G = int(np.ceil(np.sqrt(total)))
    cell = np.arange(total)
    corner = np.array([(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)])
    uv_all = ((np.stack([cell % G, cell // G], axis=1)[:, None, :] + corner[None]) / G).astype(np.float32)
    uvs = {m: uv_all[sum(prims[:m]):sum(prims[:m + 1])] for m in range(len(prims))}
    d, _ = prt_amd.bake_cosine_set(K, np.random.default_rng(K))
    w = np.full((K, 1), 1.0 / K, np.float32)
    out = {"workload": "c3_sponza_standin", "layout": f"{total} triangles, one cell each of a {G} x {G} grid, {W} x {W} atlas", "K": K,
           "reps": args.reps, "device": t.device_info()[0], "compute_units": t.device_info()[1], "scene_radius": radius,
           "source_sha16": prt_amd.loaded_source_sha16(), "visibility": {}}
    sync = lambda: t.stats()  # noqa: E731  (prt_hip_get_stats synchronises the context's stream)

    def wall(call):
        sync()
        t0 = time.perf_counter()
        call()
        st = sync()
        return (time.perf_counter() - t0) * 1e3, st["kernelMs"]

    with prt_amd.DeviceArrays() as dev:
        d_uv = {m: dev.upload(uv) for m, uv in uvs.items()}
        d_texels, d_hits = dev.alloc(4 * W * W), dev.alloc(prt_amd.HIT_DTYPE.itemsize * W * W)
        n = t.atlas_rasterize_device(W, W, d_uv, dict(enumerate(prims)), d_texels, d_hits)["n"]
        d_points = dev.alloc(32 * n)
        t.atlas_points_async(n, W, d_texels, d_hits, d_points, bias=bias)
        sync()
        pts = np.zeros(n, prt_amd.BAKE_POINT_DTYPE)
        dev.download(pts, d_points)
        table = prt_amd.BakeSets(K=K, C=1, nSets=1, reserved=0, dirs=dev.upload(d), weights=dev.upload(w))
        d_out, d_occ = dev.alloc(4 * n), dev.alloc(n * K)
        part = (1 << 24) // K
        d_rays = dev.alloc(32 * part * K)
        out["points"], out["rays"] = n, n * K
        for label, md in (("inf", float("inf")), ("radius_over_10", radius / 10.0)):
            v = prt_amd.VisibilityParams(md, 0)
            times = {k: [] for k in ("a_bake_visibility_wall", "a_vis_trace_kernel", "a_vis_reduce_wall", "b_query_any_kernels", "c_bake_rays_wall")}
            fused = lambda: t.bake_visibility_async(n, d_points, table, d_out, max_distance=md, d_occluded=d_occ)  # noqa: E731
            reduce_ = lambda: t._chk(L.prt_hip_bake_visibility_reduce(ctx, n, d_points, C.byref(table), C.byref(v), d_occ, d_out, 0, None), "reduce")  # noqa: E731
            for rep in range(2 + args.reps):
                a_wall, a_kernel = wall(fused)
                r_wall, _ = wall(reduce_)
                if rep >= 2:
                    times["a_bake_visibility_wall"].append(a_wall)
                    times["a_vis_trace_kernel"].append(a_kernel)
                    times["a_vis_reduce_wall"].append(r_wall)
            occ = np.zeros(n * K, np.uint8)
            dev.download(occ, d_occ)
            ao = np.zeros(n, np.float32)
            dev.download(ao, d_out)
            # (b) and (c): the rays of every part once, tMax written on the host, then the repetitions of query_any on them
            b_sum, c_sum, equal = np.zeros(2 + args.reps), np.zeros(2 + args.reps), True
            for i0 in range(0, n, part):
                m = min(part, n - i0)
                rays_call = lambda: t._chk(L.prt_hip_bake_rays(ctx, m, d_points + 32 * i0, C.byref(table), d_rays, 0, None), "bake_rays")  # noqa: E731
                for rep in range(2 + args.reps):
                    c_sum[rep] += wall(rays_call)[0]
                rays = np.zeros(m * K, prt_amd.RAY_DTYPE)
                dev.download(rays, d_rays)
                rays["tMax"] = np.float32(md)
                dev.upload(rays, d_rays)
                d_any = dev.alloc(m * K)
                for rep in range(2 + args.reps):
                    b_sum[rep] += wall(lambda: t.query_any_async(m * K, d_rays, d_any))[1]
                got = np.zeros(m * K, np.uint8)
                dev.download(got, d_any)
                equal = equal and got.tobytes() == occ[i0 * K:(i0 + m) * K].tobytes()
            times["b_query_any_kernels"], times["c_bake_rays_wall"] = list(b_sum[2:]), list(c_sum[2:])
            med = {k: float(np.median(x)) for k, x in times.items()}
            res = {"maxDistance": md, "ms": {k: spread(x) for k, x in times.items()}, "occluded_fraction": float(occ.mean()),
                   "mean_visibility": float(ao.mean()), "bytes_equal_query_any": equal,
                   "vis_trace_over_b_plus_c": med["a_vis_trace_kernel"] / (med["b_query_any_kernels"] + med["c_bake_rays_wall"]),
                   "vis_trace_minus_b_plus_c_ms": med["a_vis_trace_kernel"] - (med["b_query_any_kernels"] + med["c_bake_rays_wall"]),
                   "spread_of_b_ms": float(np.max(times["b_query_any_kernels"]) - np.min(times["b_query_any_kernels"])),
                   "mrays_per_s": {"a_end_to_end": n * K / med["a_bake_visibility_wall"] / 1e3, "a_vis_trace_kernel": n * K / med["a_vis_trace_kernel"] / 1e3,
                                   "b_query_any": n * K / med["b_query_any_kernels"] / 1e3}}
            if label == "inf":  # (d) the host-array route, once
                t0 = time.perf_counter()
                sums, same = [], True
                for i0 in range(0, n, part):
                    p = pts[i0:i0 + part]
                    r = t.bake_rays(p["P"], p["N"], d, bias=p["bias"])
                    r["tMax"] = np.float32(md)
                    o = t.query_any(r["org"], r["dir"], r["tMax"])
                    same = same and o.tobytes() == occ[i0 * K:(i0 + len(p)) * K].tobytes()
                    sums.append(((o.reshape(len(p), K) == 0) * w[:, 0]).sum(axis=1, dtype=np.float32))
                res["d_host_route_ms"] = (time.perf_counter() - t0) * 1e3
                res["d_bytes_equal"] = same
                res["d_largest_difference_of_the_numpy_sum"] = float(np.abs(np.concatenate(sums) - ao).max())
                res["d_over_a"] = res["d_host_route_ms"] / med["a_bake_visibility_wall"]
            out["visibility"][label] = res
    t.close()
    emit(out, args.out)


def host_rays(pts, d):
    """What a baker wrote in numpy: a tangent frame per point, the K directions rotated into it, the origin tiled."""
    N = pts["N"].astype(np.float64)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    u = np.where((np.abs(N[:, 0]) > 0.1)[:, None], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0])
    T = np.cross(N, u)
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    B = np.cross(T, N)
    dirs = d[None, :, 0, None] * B[:, None, :] + d[None, :, 1, None] * T[:, None, :] + d[None, :, 2, None] * N[:, None, :]
    org = np.repeat(pts["P"] + np.float32(1e-4) * pts["N"], d.shape[0], axis=0)
    return prt_amd.make_rays(org, dirs.reshape(-1, 3), 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--out", default=None)
    ap.add_argument("--radiance", action="store_true")
    ap.add_argument("--bake", action="store_true")
    ap.add_argument("--atlas", action="store_true")
    ap.add_argument("--lens", action="store_true")
    ap.add_argument("--atlas-filter", action="store_true")
    ap.add_argument("--visibility", action="store_true")
    ap.add_argument("--ref-spp", type=int, default=2040)
    args = ap.parse_args()
    prt_amd.build()
    if args.radiance:
        return radiance(args)
    if args.bake:
        return bake(args)
    if args.atlas:
        return atlas(args)
    if args.atlas_filter:
        return atlas_filter(args)
    if args.lens:
        return lens(args)
    if args.visibility:
        return visibility(args)
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
