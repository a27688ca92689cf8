"""What a scene edit costs next to the full upload it replaces (include/prt_hip.h "scene edits").  Workload: the C3 stand-in
(setup_atrium_standin(1920, 1080)) under a 2048 x 1024 sky map.  Every figure is host wall clock over the call, its
synchronisation included (the upload's copies are synchronous; a stats read drains the stream before each timing); median and spread
(max - min) of --reps repetitions, edit and yardstick ALTERNATING within the run.  The yardstick is what the library offered before
the edit calls: Scene.set_infinite_area_light (which rebuilds both tables on the host) + upload_scene for a new map, upload_scene
alone for the rest.  Also the HIP-event times of the two kernels (prt_hip_test_edit_profile).  Diagnostic; prints one line per row."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import prt_amd  # noqa: E402
import prt_testlib as T  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tris", type=int, default=262000)
    ap.add_argument("--env", type=int, nargs=2, default=(2048, 1024))
    a = ap.parse_args()
    prt_amd.build()
    scene, camera, _ = prt_amd.setup_atrium_standin(1920, 1080, tris=a.tris)
    envs = [T.sky_env(a.env[0], a.env[1], seed=s) for s in (7, 8)]
    scene.set_infinite_area_light(envs[0])
    t = prt_amd.PathTracer(test_entry_points=True)
    t.upload_scene(scene)
    t.set_camera(camera)
    arr = scene.arrays()
    mats = arr["meshes"][0]["materials"]
    alpha = sorted((i for i in set(int(m) for m in mats["diffuseMap"][mats["alphaTest"] != 0])), key=lambda i: -arr["textures"][i].size)[0]
    texels = [arr["textures"][alpha], np.ascontiguousarray(arr["textures"][alpha][::-1])]
    print(f"scene: {scene.describe().contents.meshes[0].primCount} triangles, {len(arr['textures'])} textures ({sum(x.size for x in arr['textures'])} bytes), "
          f"environment map {a.env[0]} x {a.env[1]}; alpha-tested texture {alpha}: {arr['textures'][alpha].shape}; library {prt_amd.test_lib().prt_hip_source_sha16().decode()}")

    def drain():
        prt_amd.hip_runtime().hipDeviceSynchronize()

    def env_edit(k):
        scene.set_infinite_area_light(envs[k % 2])  # (the host mirror builds its tables here; the edit does not send them)
        drain()
        return timed(lambda: t.update_lights(scene))

    def env_full(k):
        drain()
        return timed(lambda: (scene.set_infinite_area_light(envs[k % 2]), t.upload_scene(scene)))

    def sun_edit(k):
        scene.set_directional_light(prt_amd._normalize((0.05 + 0.01 * k, 1.0, 0.1)), (16.7, 15.6, 11.7))
        scene.set_infinite_area_light(envs[0])
        drain()
        return timed(lambda: t.update_lights(scene, env=False))

    def mat_edit(k):
        m = mats[1].copy()
        m["diffuse"] = (0.1 * (k % 7), 0.5, 0.5)
        scene.set_material(0, 1, m)
        drain()
        return timed(lambda: t.update_materials(scene, [(0, 1)]))

    def tex_edit(k):
        scene.set_texture_texels(alpha, texels[k % 2])
        drain()
        return timed(lambda: t.update_textures(scene, [alpha]))

    def full(k):
        drain()
        return timed(lambda: t.upload_scene(scene))

    rows = [("update_lights, new map", env_edit, "set_infinite_area_light + upload_scene", env_full),
            ("update_lights, ENV_KEEP", sun_edit, "upload_scene", full),
            ("update_materials, one material", mat_edit, "upload_scene", full),
            (f"update_textures, texture {alpha}", tex_edit, "upload_scene", full)]
    for name, edit, yname, yard in rows:
        edit(0), yard(1)  # warm-up of both sides
        e, y = [], []
        for k in range(a.reps):
            e.append(edit(2 * k))
            y.append(yard(2 * k + 1))
        me, my = float(np.median(e)), float(np.median(y))
        print(f"{name:36s} median {me:9.3f} ms spread {max(e) - min(e):8.3f} [{', '.join(f'{v:.3f}' for v in e)}]")
        print(f"  {yname:34s} median {my:9.3f} ms spread {max(y) - min(y):8.3f} [{', '.join(f'{v:.3f}' for v in y)}]   ratio {my / me:.1f}")
    d = scene.describe().contents.textures[alpha]
    up = prt_amd.TextureUpdate(alpha, d.width, d.height, d.component, d.texels)
    ms = (C.c_float * 2)()
    t._chk(t._L.prt_hip_test_edit_profile(t._ctx, 1, C.byref(up), a.reps, ms), "prt_hip_test_edit_profile")
    print(f"HIP events, median of {a.reps}: environment tables {a.env[0]} x {a.env[1]} (rows + column kernel) {ms[0]:.3f} ms; "
          f"alpha classes of {d.width} x {d.height} cells {ms[1]:.4f} ms")
    t.close()


if __name__ == "__main__":
    main()
