"""The shell the ray-batch kernels share (prt_amd/csrc/prt_batch.h: gbuffer_kernel, position_kernel, the query kernels and the test
build's rays_kernel behind trace_batch; prt_batch_begin / prt_batch_end on the host): which launches the statistics count and time,
and the block edges of the shared launch.  Cornell box with the teapot, a 64 x 48 camera, the test build, one context per test;
everything at tolerance 0."""
import numpy as np
import pytest

import prt_amd
import prt_testlib as T

pytestmark = pytest.mark.gpu
W, H = 64, 48
BLOCK = 1024  # PRT_BLOCK: threads of a workgroup, one ray each


@pytest.fixture
def box():
    prt_amd.build()
    scene, camera, _ = prt_amd.setup_cornell_box(W, H, teapot_mesh=T.teapot_product_mesh())
    t = prt_amd.PathTracer(test_entry_points=True)
    t.upload_scene(scene)
    t.set_camera(camera)
    t.scene = scene  # (the context reads the scene's arrays only during the upload; kept for the test's own use)
    t.rays = lambda n: prt_amd.pixel_centre_rays(camera.desc, np.arange(n) % W, np.arange(n) // W)
    yield t
    t.close()


def test_guide_launches_stay_out_of_the_statistics(box):
    """The G-buffer and the position guide clear the counters and are not timed; a batch of the caller's rays is."""
    r = box.rays(8)
    box.query_nearest(r["org"], r["dir"], r["tMax"])
    st = box.stats()
    assert st["kernelLaunches"] == 1 and st["raysTraced"] == 8  # something to consume, and to clear
    box.gbuffer(0)
    st = box.stats()
    assert (st["kernelLaunches"], st["raysTraced"], st["stackOverflow"]) == (0, 0, 0), st
    box.query_nearest(r["org"], r["dir"], r["tMax"])
    assert box.stats()["raysTraced"] == 8
    pos = box.denoise_position()  # stale: one launch of position_kernel
    st = box.stats()
    assert (st["kernelLaunches"], st["raysTraced"], st["stackOverflow"]) == (0, 0, 0), st
    every = box.rays(W * H)  # the guide's own rays: its distances are the query's, so the plane is this launch's answer
    near = box.query_nearest(every["org"], every["dir"], every["tMax"])
    assert (near["t"] != -1).any() and pos[..., 3].reshape(-1).tobytes() == near["t"].tobytes()
    assert box.stats()["kernelLaunches"] == 1
    box.trace_rays(0, r["org"], r["dir"], 1e5)
    st = box.stats()
    assert st["kernelLaunches"] == 1 and st["kernelMs"] > 0 and st["stackOverflow"] == 0, st


@pytest.mark.parametrize("n", [8, BLOCK + 8])
def test_row_level_batches_equal_the_queries_at_the_block_edges(box, n):
    """n = 8: one workgroup with 8 busy lanes; n = 1032: a second workgroup with one packet of work."""
    r = box.rays(n)
    org, d = r["org"], r["dir"]
    near = box.query_nearest(org, d, 1e5)
    anyhit = box.query_any(org, d, 1e5)
    m0, m1, m2, m3 = (box.trace_rays(mode, org, d, 1e5) for mode in range(4))
    hit = near["t"] != -1
    assert hit.any() and anyhit.any()
    assert m0[hit].tobytes() == near[hit].tobytes()
    assert (m0["t"][~hit] == -1).all()
    assert ((m2["t"] == 1) == (anyhit == 1)).all() and np.isin(m2["t"], (0, 1)).all()
    assert ((m1["t"] != -1) == hit).all()
    assert ((m3["t"] == 1) == (anyhit == 1)).all()
    assert box.stats()["stackOverflow"] == 0


@pytest.mark.parametrize("n", [1, BLOCK + 1])
def test_fused_surface_records_equal_the_two_step_query(box, n):
    r = box.rays(n)
    hits, surf = box.query_nearest(r["org"], r["dir"], r["tMax"], surface=True)
    assert (hits["t"] != -1).any() == (n > 1)  # the corner pixel's ray passes the box: the batch of one is a miss record
    assert hits.tobytes() == box.query_nearest(r["org"], r["dir"], r["tMax"]).tobytes()
    assert surf.tobytes() == box.query_surface(r["org"], r["dir"], hits).tobytes()
    assert box.query_get_counts() == 0
