"""The bounce loop (shade_round, prt_amd/csrc/prt_frame.h) under hostile materials and lights on the MI355X; the scenes are those of
tests/prt_hostile_shade.py and the CPU half is tests/test_hostile_shade_cpu.py.  Everything is BIT-EXACT (tolerance 0; "is NaN" where the
other side has a NaN): the images of both builds, raysTraced and occludedTraced, and the counting build's event counts -- through
check_scene of test_gpu_shadow_skip.py.

  FIXTURE scenes  the product = the live oracle = the COMPILED reference's image and ray counts in tests/golden/hostile_shade.npz
  PRODUCT scenes  refraction (a zero scatter direction in every bounce: a counted ray that misses) and specular patches under hostile
                  suns, against the live oracle at depth caps 1, 5, 14 and Russian roulette from depth 0 and 4
  the tally       no occlusion ray is answered without a walk under a NaN or infinite intensity; some are under the plain sun
  progressive     two passes = one render, and the accumulator's sums of both builds are equal (a pass is 8 samples at least)
  scene edits     update_materials / update_lights to the hostile values = the fixture image of the freshly uploaded scene
Which of these tests fail under std_max's arguments swapped, fmaxf, `> 0` for `!= 0` and a skip rule without finite3(I):
profiles/r19_hostile_shade.txt, section C."""
import numpy as np
import pytest

import prt_hostile_shade as S
import prt_testlib as T
from prt_gpucases import check_scene
from prt_gpukit import assert_same_image, upload
from prt_gpukit import gpu_event_accounting  # noqa: F401  (fixture: the oracle's any-hit accounting)
from prt_gpukit import rows as tracer  # noqa: F401  (fixture: this module's tracer is a context of the test build)

pytestmark = pytest.mark.gpu
DEPTH = 14  # the reference's literal


@pytest.fixture(autouse=True)
def roulette_depth_restored(tracer):
    yield
    set_rr_depth(tracer, 4)


def set_rr_depth(tracer, depth):
    tracer.rr_depth = depth
    T.oracle().orc_set_rr_depth(depth)


_checked = {}


def checked(tracer, name):
    """check_scene of a FIXTURE scene at the fixture's settings, once per module: (oracle stats, rays skipped, the oracle's image)."""
    if name not in _checked:
        scene, camera = S.scene(name)
        _checked[name] = check_scene(tracer, scene, camera, S.SPP, DEPTH, name)
    return _checked[name]


def render_equals_fixture(tracer, name, what):
    g = S.golden(name)
    for count in (False, True):
        img = tracer.render(S.SPP, max_depth=DEPTH, count_traffic=count)
        assert_same_image(img, g["image"], f"{what}, count_traffic={count}")
        st = tracer.last_stats
        assert (st["raysTraced"], st["occludedTraced"]) == g["rays"], (what, st, g["rays"])


@pytest.mark.parametrize("name", S.FIXTURE)
def test_fixture_scene_equals_the_reference_and_the_oracle(tracer, name):
    ost, skipped, ref = checked(tracer, name)  # product = oracle: images of both builds, ray counts, the counting build's event counts
    g = S.golden(name)
    assert_same_image(ref, g["image"], name + ": the oracle against the fixture")
    assert (ost["raysTraced"], ost["occludedTraced"]) == g["rays"], (name, ost, g["rays"])
    render_equals_fixture(tracer, name, name)  # (check_scene left the scene uploaded)


def test_no_ray_is_skipped_under_a_non_finite_intensity(tracer):
    """The stage has surfaces that face away from every sun here (the patch with the flipped shading normal; under the light from below,
    everything): the rule answers their rays without a walk only while an unoccluded answer would add +-0, and 0 * NaN or 0 * inf is NaN."""
    for name in ("light_nan", "light_inf_below"):
        ost, skipped, ref = checked(tracer, name)
        assert ost["occludedTraced"] > 0 and skipped == 0, (name, skipped)
        assert np.isnan(ref).any(), name
    ost, skipped, _ = checked(tracer, "rr")
    assert 0 < skipped < ost["occludedTraced"], (skipped, ost["occludedTraced"])
    ost, skipped, _ = checked(tracer, "box_inf")  # a finite light, but slots whose beta is infinite are traced
    assert 0 < skipped < ost["occludedTraced"], (skipped, ost["occludedTraced"])


@pytest.mark.parametrize("rr_depth", [0, 4])
@pytest.mark.parametrize("max_depth", [1, 5, 14])
@pytest.mark.parametrize("name", S.PRODUCT + ("rr", "nonfinite", "box_nan"))
def test_depth_caps_and_roulette_from_the_first_bounce_match_the_oracle(tracer, name, max_depth, rr_depth):
    """With rr_depth 0 the roulette meets every hostile beta from the first bounce (|beta| = 0.95 and 1 exactly on the K95 and K1
    patches).  The PRODUCT scenes exist only here: refraction at a first hit and behind a bounce, specular slots that carry a hostile
    light from bounce to bounce."""
    set_rr_depth(tracer, rr_depth)
    scene, camera = S.scene(name)
    ost, _, ref = check_scene(tracer, scene, camera, S.SPP, max_depth, f"{name}, depth cap {max_depth}, roulette past {rr_depth}")
    assert ost["raysTraced"] > scene_pixels(name) * S.SPP and float(np.nansum(np.abs(ref))) > 0


def scene_pixels(name):
    _, _, w, h = S.BOX_CAMERA if name in S.BOXES else S.STAGE_CAMERA
    return w * h


def test_refraction_sends_one_counted_ray_that_misses(tracer):
    """The definition in include/prt_hip.h, rendered: on a stage whose every material refracts and emits (1, 2, 3), without a light, a path
    is its camera ray, its emission and one scatter ray that misses -- at every depth cap."""
    scene, camera = S.scene("refract_first", light=None)
    value = S.material_array([S._m(0.5, (1.0, 2.0, 3.0), refl=2)])[0]
    d = scene.describe().contents
    for m in range(d.meshCount):
        for k in range(d.meshes[m].materialCount):
            scene.set_material(m, k, value)
    upload(tracer, scene, camera)
    n = camera.width * camera.height * S.SPP
    one = tracer.render(S.SPP, max_depth=1)
    st1 = tracer.last_stats
    hits = st1["raysTraced"] - n
    assert 0 < hits < n and st1["occludedTraced"] == 0
    deep = tracer.render(S.SPP, max_depth=DEPTH)
    assert tracer.last_stats["raysTraced"] == n + hits and deep.tobytes() == one.tobytes()
    assert (one[..., 1] == 2 * one[..., 0]).all() and float(one.astype(np.float64).sum()) == 6.0 * hits / 8
    ref, ost = T.OracleScene(T.scene_desc_from_product(scene, camera, 1.0)).render(S.SPP, max_depth=DEPTH)
    assert_same_image(deep, ref, "all-refraction stage")
    assert ost["raysTraced"] == n + hits


@pytest.mark.parametrize("name", ["nonfinite", "box_rr"])
def test_two_passes_equal_one_render_and_both_builds_keep_the_same_sums(tracer, name):
    """accumulate(8) twice = render(16) = the oracle's 16 spp (8 samples, one packet per pixel, is the smallest pass), and the accumulator's
    sums of the timed and the counting build are equal word for word outside NaN."""
    scene, camera = S.scene(name)
    upload(tracer, scene, camera)
    ref, ost = T.OracleScene(T.scene_desc_from_product(scene, camera, 1.0)).render(2 * S.SPP, max_depth=DEPTH)
    once = tracer.render(2 * S.SPP, max_depth=DEPTH)
    assert_same_image(once, ref, name + ": render(16)")
    assert tracer.last_stats["raysTraced"] == ost["raysTraced"]
    sums = {}
    for count in (False, True):
        tracer.accum_reset()
        rays = 0
        for _ in range(2):
            img = tracer.accumulate(S.SPP, max_depth=DEPTH, count_traffic=count)
            rays += tracer.last_stats["raysTraced"]
        assert_same_image(img, ref, f"{name}: two passes of 8, count_traffic={count}")
        assert rays == ost["raysTraced"], (name, rays, ost["raysTraced"])
        sums[count] = tracer.accum_export()["sum"]
    assert_same_image(sums[False], sums[True], name + ": the accumulator's sums of both builds")
    if name == "nonfinite":
        assert not np.isfinite(sums[True]).all()


@pytest.mark.parametrize("name", ["nonfinite", "emit"])
def test_update_materials_to_hostile_values_equals_a_fresh_upload(tracer, name):
    scene, camera = S.scene("plain")
    upload(tracer, scene, camera)
    tracer.render(S.SPP, max_depth=DEPTH)
    mats = S.material_array(S.stage_materials(name))
    for k in range(len(mats)):
        scene.set_material(0, k, mats[k])
    tracer.update_materials(scene, [(0, k) for k in range(len(mats))])
    render_equals_fixture(tracer, name, f"plain stage edited into {name}")


@pytest.mark.parametrize("name", ["light_zero", "light_unnorm", "light_neg", "light_nan", "light_inf_below"])
def test_update_lights_to_a_hostile_sun_equals_a_fresh_upload(tracer, name):
    scene, camera = S.scene(name, light="sun")
    upload(tracer, scene, camera)
    tracer.render(S.SPP, max_depth=DEPTH)
    scene.set_directional_light(*S.LIGHTS[S.STAGES[name][2]])
    tracer.update_lights(scene)
    render_equals_fixture(tracer, name, f"sun edited into {name}")
