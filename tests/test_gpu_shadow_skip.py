"""Occlusion rays whose answer cannot reach the image are answered without a walk: when the surface faces away from
the slot's light -- dot(lightDir, normal) <= 0, beta and the light's intensity finite -- an unoccluded answer would add +-0, so the
timed build neither queues nor walks the ray.  Everything here is BIT-EXACT against the oracle (tolerance 0; "is NaN" where the
oracle has a NaN, as bench.py compares): the images, the ray counts (which stay the reference's: a skipped ray is still counted), and
-- with count_traffic, which walks every ray -- the box and triangle tests.  The tally of skipped rays comes from the test build of the
library (include/prt_hip_test.h)."""
import numpy as np
import pytest

import prt_amd
import prt_testlib as T
from prt_gpucases import check_scene
from prt_gpukit import assert_same_image, upload
from prt_gpukit import gpu_event_accounting  # noqa: F401  (fixture)
from prt_gpukit import rows as tracer  # noqa: F401  (fixture: this module's tracer is a context of the test build, for the tally's entry point)

pytestmark = pytest.mark.gpu


def quad_mesh(kd=(0.7, 0.6, 0.5), half=1.5, normals=None):
    """One diffuse quad in the plane y = 0 whose geometric normal, normalize(cross(p1 - p0, p2 - p0)), is +y."""
    pos = np.array([(-half, 0, half), (half, 0, half), (half, 0, -half), (-half, 0, -half)], dtype=np.float32)
    idx = np.array([(0, 1, 2), (0, 2, 3)], dtype=np.uint32)
    assert np.all(np.cross(pos[1] - pos[0], pos[2] - pos[0]) == (0, 4 * half * half, 0))
    mats = np.array([T.make_material(diffuse=kd)], dtype=T.MATERIAL_DTYPE)
    m = prt_amd.Mesh.from_arrays(idx, pos, np.zeros(2, np.uint32), mats.view(prt_amd.MATERIAL_DTYPE), normals=normals)
    m.calculate_bounds()
    return m


def quad_scene(light_dir, intensity=(3.0, 2.5, 2.0), normals=None):
    scene = prt_amd.Scene()
    scene.add(quad_mesh(normals=normals))
    scene.set_directional_light(light_dir, intensity)
    # the quad fills the middle of the 32x32 image: packets with 8, with a few and with no path alive
    camera = prt_amd.Camera().create((0.0, 2.0, 3.0), (0.0, -0.6, -1.0), 32, 32)
    return scene, camera


def test_atrium_image_counts_and_tally(tracer):
    """C3's scene class at a test size: 20 000 triangles, 64x36, 16 spp, depth cap 8, the directional light of the flagship workload."""
    scene, camera, exposure = prt_amd.setup_atrium_standin(64, 36, tris=20000)
    ost, skipped, ref = check_scene(tracer, scene, camera, 16, 8, "atrium 64x36", exposure)
    assert 0 < skipped < ost["occludedTraced"], (skipped, ost["occludedTraced"])


@pytest.mark.parametrize("name,light_dir,expect", [("light from below", (0.0, -1.0, 0.0), "all"), ("light from above", (0.0, 1.0, 0.0), "none"),
                                                   ("light parallel to the quad", (1.0, 0.0, 0.0), "all")])
def test_known_counts_on_one_quad(tracer, name, light_dir, expect):
    """One upward-facing diffuse quad, no vertex normals, no bump map: the shading normal is (0, 1, 0) everywhere, every scatter ray
    leaves the scene, so every occlusion ray belongs to a first hit and the dot product is the light direction's y: -1, 1 and -- the
    light exactly in the quad's plane -- a zero, which the rule includes."""
    scene, camera = quad_scene(light_dir)
    ost, skipped, ref = check_scene(tracer, scene, camera, 8, 14, "quad, " + name)
    assert ost["occludedTraced"] > 0
    assert skipped == (ost["occludedTraced"] if expect == "all" else 0), (name, skipped, ost["occludedTraced"])


def test_excluded_cases_are_traced_and_match(tracer):
    """What the rule excludes can give a NaN in the reference and is therefore traced: an infinite intensity (0 * inf) under a light
    from below, and a NaN shading normal (a NaN dot product)."""
    scene, camera = quad_scene((0.0, -1.0, 0.0), intensity=(np.inf, 1.0, 1.0))
    ost, skipped, ref = check_scene(tracer, scene, camera, 8, 14, "quad, light from below with intensity (inf, 1, 1)")
    assert ost["occludedTraced"] > 0 and skipped == 0, skipped
    assert np.isnan(ref).any(), "the infinite intensity must reach the image as NaN"

    n = np.tile(np.array([(0.0, 1.0, 0.0)], dtype=np.float32), (4, 1))
    n[0] = 0.0  # a degenerate vertex normal: interpolated normals of length 0 near this corner normalise to NaN ... and
    n[2] = np.nan  # ... a NaN vertex normal makes every normal of both triangles NaN
    scene, camera = quad_scene((0.0, -1.0, 0.0), normals=n)
    ost, skipped, ref = check_scene(tracer, scene, camera, 8, 14, "quad with degenerate vertex normals")
    assert ost["occludedTraced"] > 0 and skipped == 0, skipped
    assert np.isnan(ref).any(), "the NaN normal must reach the image"


def dark_box_scene():
    """The inside of a closed dark box (kd 0.05), every face's normal pointing inwards, the light below and outside it."""
    c = np.array([(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32)  # corner x*4 + y*2 + z
    faces = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    idx = []
    for f in faces:
        p = c[list(f)]
        inward = np.dot(np.cross(p[1] - p[0], p[2] - p[0]), -p.mean(0)) > 0
        a, b, cc, d = f if inward else f[::-1]
        idx += [(a, b, cc), (a, cc, d)]
    idx = np.array(idx, dtype=np.uint32)
    mats = np.array([T.make_material(diffuse=(0.05, 0.05, 0.05))], dtype=T.MATERIAL_DTYPE)
    m = prt_amd.Mesh.from_arrays(idx, c, np.zeros(len(idx), np.uint32), mats.view(prt_amd.MATERIAL_DTYPE))
    m.calculate_bounds()
    scene = prt_amd.Scene()
    scene.add(m)
    scene.set_directional_light(prt_amd._normalize((0.2, -1.0, 0.1)), (16.7, 15.6, 11.7))
    camera = prt_amd.Camera().create((0.0, 0.0, 0.9), (0.0, -0.2, -1.0), 32, 32)
    return scene, camera


def test_a_round_that_emits_nothing_makes_the_group_ready(tracer):
    """Past the Russian-roulette depth a dark box loses every path of a packet in rounds whose occlusion rays are all skipped (floor
    and two walls face away from the light): such a round emits no ray at all, and the group must be picked up again at once -- a
    group left waiting would end the launch through the watchdog (PrtError), not hang it."""
    scene, camera = dark_box_scene()
    ost, skipped, ref = check_scene(tracer, scene, camera, 16, 12, "dark box")
    assert 0 < skipped < ost["occludedTraced"], (skipped, ost["occludedTraced"])


def test_single_ray_occlusion_queue(tracer):
    """Cornell box + specular teapot under a directional light, depth 4: packets with one or two paths alive send their occlusion
    rays through the single-ray queue."""
    scene, camera, exposure = prt_amd.setup_cornell_box(64, 64, teapot_mesh=T.teapot_product_mesh())
    scene.set_directional_light(prt_amd._normalize((0.2, 1.0, 0.2)), (16.7, 15.6, 11.7))
    ost, skipped, ref = check_scene(tracer, scene, camera, 8, 4, "Cornell + teapot + light", exposure)
    assert 0 < skipped < ost["occludedTraced"], (skipped, ost["occludedTraced"])


@pytest.mark.parametrize("teapot", [False, True])
def test_environment_light(tracer, teapot):
    """The scene of tests/golden/env_light.npz (Cornell box under the seeded sky map) at 48x48, 8 spp: a diffuse slot samples its light
    in the bounce that emits the ray and is skipped by the rule; with the specular teapot, slots also carry the light of an EARLIER
    bounce, whose direction is not in registers: those are traced as before."""
    scene, camera, exposure = prt_amd.setup_cornell_box(48, 48, teapot_mesh=T.teapot_product_mesh() if teapot else None)
    scene.set_infinite_area_light(T.sky_env(64, 32))
    ost, skipped, ref = check_scene(tracer, scene, camera, 8, 14, "env-lit Cornell" + (" + teapot" if teapot else ""), exposure)
    assert 0 < skipped < ost["occludedTraced"], (skipped, ost["occludedTraced"])


def test_accumulate_and_adaptive_passes_see_the_same_packet_sums(tracer):
    """One pass through the progressive API equals the one-shot render, and the accumulator's sums and the adaptive pass's Welford
    moments are those of the counting build, which skips nothing: both builds hand the same packet sums to them."""
    scene, camera, exposure = prt_amd.setup_atrium_standin(64, 36, tris=20000)
    upload(tracer, scene, camera)
    desc = T.scene_desc_from_product(scene, camera, exposure)
    ref, ost = T.OracleScene(desc).render(16, max_depth=8)
    state = {}
    for count in (False, True):
        tracer.accum_reset()
        img = tracer.accumulate(16, exposure=exposure, max_depth=8, count_traffic=count)
        assert_same_image(img, ref, f"accumulate pass, count_traffic={count}")
        assert tracer.last_stats["occludedTraced"] == ost["occludedTraced"]
        assert (tracer.occlusion_skipped() > 0) == (not count)
        acc = tracer.accum_export()
        tracer.accum_reset()
        img, active = tracer.adaptive_pass(16, 0.01, 16, 64, exposure=exposure, max_depth=8, count_traffic=count)
        assert active == 64 * 36
        assert_same_image(img, ref, f"adaptive pass, count_traffic={count}")
        assert (tracer.occlusion_skipped() > 0) == (not count)
        state[count] = (acc["sum"], tracer.accum_export()["sum"], tracer.accum_export_moments())
    for a, b, what in zip(state[False], state[True], ("accumulator sums", "adaptive pass's sums", "Welford moments")):
        assert a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes(), what
