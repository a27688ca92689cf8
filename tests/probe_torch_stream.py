"""Child process of tests/test_gpu_probe.py::test_device_tensors_on_a_callers_stream: prt_hip_query_radiance on torch tensors on a
non-default torch stream, behind a kernel that writes the rays and in front of one that reads the radiance, against the host path.
A process of its own because torch has to be imported FIRST: it loads the HIP runtime it ships, and the library then binds to that
one (as in bench.py); a process that has already loaded the library would end up with two runtimes.  Prints "ok <n> probes"."""
import os
import sys

import torch  # noqa: E402  (before prt_amd: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import prt_amd  # noqa: E402
import prt_hostile_shade as HS  # noqa: E402
import prt_probe_ref as PR  # noqa: E402


def main():
    n, spp, seed = 3000, 8, 808
    scene, _ = HS.scene("plain", light=None)
    scene.set_infinite_area_light(HS.sky())
    t = prt_amd.PathTracer(max_depth=8)
    t.upload_scene(scene)
    org, d = PR.stage_probes(n, seed=23)
    want = t.query_radiance(org, d, spp, seed=seed)
    assert (want != 0).any(axis=1).sum() > n // 4
    rays = prt_amd.make_rays(org, d, 0.0)
    dev = torch.device("cuda", 0)
    src = torch.from_numpy(rays.view(np.float32).reshape(n, 8).copy()).to(dev)
    half = src * 0.5
    torch.cuda.synchronize()
    t.stats()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        d_rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        d_rad = torch.full((n, 3), float("nan"), dtype=torch.float32, device=dev)
        assert d_rays.data_ptr() % 16 == 0
        torch.add(half, half, out=d_rays)  # the kernel that writes the rays: x * 0.5 + x * 0.5 is x bit for bit (no NaN, nothing denormal)
        t.query_radiance_async(n, d_rays.data_ptr(), d_rad.data_ptr(), spp, seed=seed, stream=s.cuda_stream)
        doubled = d_rad * 2.0              # the kernel that reads the radiance
    s.synchronize()
    assert torch.equal(d_rays, src), "the rays the kernel wrote"
    got = d_rad.cpu().numpy()
    assert got.tobytes() == want.tobytes(), f"{int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())} of {n} probes differ from the host path"
    assert doubled.cpu().numpy().tobytes() == (want * np.float32(2.0)).tobytes(), "the kernel behind the query read other radiance"
    st = t.stats()
    assert st["nPx"] == n and st["kernelLaunches"] == 1, st
    t.close()
    print(f"ok {n} probes")


if __name__ == "__main__":
    main()
