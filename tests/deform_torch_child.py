"""Child process of tests/test_gpu_deform.py::test_torch_tensor_on_torchs_stream: torch computes the new positions on the GPU, on a
non-default torch stream, and prt_hip_deform_meshes reads the tensor through data_ptr() on that stream, with no synchronisation in
between; the context then equals one that uploaded the Scene updated on the host.  A process of its own because torch has to be
imported FIRST: it loads the HIP runtime it ships, and the library then binds to that one (as in bench.py).  Prints "ok deform <V>"."""
import os
import sys

import torch  # noqa: E402  (before prt_amd: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import prt_amd  # noqa: E402
import prt_deform_ref as D  # noqa: E402
import prt_testlib as T  # noqa: E402

ARRAYS = ("wnodes", "hot", "tris", "shade", "bump", "root_boxes", "radius")


def main():
    scene, camera, _ = prt_amd.setup_cornell_box(64, 64, teapot_mesh=T.teapot_product_mesh())
    tea = scene.arrays()["meshes"][1]
    offset = np.array([0.25, 0.0625, -0.125], dtype=np.float32)
    P = (tea["positions"] + offset).astype(np.float32)  # what torch's f32 add gives, element for element
    t, twin = prt_amd.PathTracer(test_entry_points=True), prt_amd.PathTracer(test_entry_points=True)
    t.upload_scene(scene)
    t.set_camera(camera)
    dev = torch.device("cuda", 0)
    base, off = torch.from_numpy(tea["positions"].copy()).to(dev), torch.from_numpy(offset).to(dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        moved = base + off  # the kernel that writes the positions
        t.deform_meshes([(1, moved, prt_amd.MeshDeform.NORMALS_RECOMPUTE)], stream=s.cuda_stream)
    s.synchronize()
    assert moved.cpu().numpy().tobytes() == P.tobytes(), "the positions torch wrote"
    gotP, gotN = t.mesh_vertices(1)
    N = D.vertex_normals(tea["indices"], P)
    assert gotP.tobytes() == P.tobytes(), "the library read other positions than torch wrote"
    assert D.bits_equal(gotN, N), "recomputed normals"
    scene.update_positions(1, P, N)
    twin.upload_scene(scene)
    twin.set_camera(camera)
    got, want = t.scene_arrays(), twin.scene_arrays()
    for k in ARRAYS:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert t.render(8).tobytes() == twin.render(8).tobytes(), "render"
    t.close()
    twin.close()
    print(f"ok deform {len(P)}")


if __name__ == "__main__":
    main()
