"""The bounce loop under hostile materials and lights without a GPU (tests/prt_hostile_shade.py): the generator reproduces the stored
arrays byte for byte and stores nothing the reference leaves undefined; the oracle's render equals the COMPILED reference's image in
tests/golden/hostile_shade.npz word for word (a NaN answers a NaN) with equal ray counts; where the reference harness is built
(oracle/_ref), ref_path_stats reproduces the committed bytes; and the stored images are not flooded: few NaN, enough finite values, every
hostile material seen, and an inf, a negative and a NaN value somewhere.

Refraction (reflectionType 2) is defined by the product, not the reference: a refraction surface scatters along a zero direction in every
bounce -- a counted ray that misses -- and the path's emission and pending light addend still count (include/prt_hip.h, DESIGN.md
"Documented deviations").  test_refraction_scatters_a_counted_ray_that_misses renders that definition with the oracle at a first hit.
Behind a bounce, where a slot takes over another path's surface with its own earlier material (path_tracer.cpp:286-288), no count can be
derived by hand: there the definition is held by the kernel, which clears the direction in every bounce by construction, against the
oracle on the scenes refract_first and refract_box (tests/test_gpu_hostile_shade.py)."""
import functools
import os

import numpy as np
import pytest

import prt_amd
import prt_hostile_shade as S
import prt_testlib as T
from prt_gpukit import assert_same_image

need_ref = pytest.mark.skipif(T.ref_binary("ref_path_stats") is None, reason="oracle/_ref/ref_path_stats is not built (no reference sources here)")


@pytest.fixture(scope="module", autouse=True)
def built():
    prt_amd.build()


@functools.lru_cache(maxsize=None)
def oracle_render(name):
    g = S.golden(name)
    return T.OracleScene(g["desc"]).render(S.SPP, seed=S.SEED)


def test_generator_reproduces_the_stored_arrays():
    z = S.golden_file()
    g = S.generate()
    stored = {k for k in z if not k.split("/")[1].startswith("ref_")}
    assert stored == set(g), stored ^ set(g)
    for k, v in g.items():
        assert v.dtype == z[k].dtype and v.shape == z[k].shape and v.tobytes() == z[k].tobytes(), k
    assert {k.split("/")[0] for k in z} == set(S.FIXTURE)
    assert S.GOLDEN_FILE.endswith("hostile_shade.npz") and os.path.getsize(S.GOLDEN_FILE) <= 256 * 1024


def test_the_fixture_holds_only_what_the_reference_defines():
    for name in S.FIXTURE:
        d = S.golden(name)["desc"]
        assert S.is_reference_defined(d), name
        assert d.env is None or (np.isfinite(d.env).all() and (d.env >= 0).all()), name
    for name in S.PRODUCT:
        assert not S.is_reference_defined(S.desc(name)), name
    assert set(S.FIXTURE) | set(S.PRODUCT) | set(S.OTHER) == set(S.STAGES) | set(S.BOXES) and not set(S.FIXTURE) & set(S.PRODUCT)
    kk = np.float32(S.K95) * np.float32(S.K95)
    assert np.sqrt(np.float32(np.float32(kk + kk) + kk)) == np.float32(0.95)


@pytest.mark.parametrize("name", S.FIXTURE)
def test_oracle_equals_the_stored_reference_image(name):
    g = S.golden(name)
    rgb, st = oracle_render(name)
    assert_same_image(rgb, g["image"], name)
    assert (st["raysTraced"], st["occludedTraced"]) == g["rays"], (name, st, g["rays"])


@need_ref
@pytest.mark.parametrize("name", S.FIXTURE)
def test_ref_path_stats_reproduces_the_committed_bytes(name):
    g = S.golden(name)
    d = g["desc"]
    rgb, st = T.ref_render(d, S.SPP, (0, 0, d.width - 1, d.height - 1), seed=S.SEED, stats=True)
    assert rgb.tobytes() == g["image"].tobytes(), name
    assert (st["raysTraced"], st["occludedTraced"]) == g["rays"], name


@pytest.mark.parametrize("name", S.FIXTURE)
def test_no_flood_hides_a_failure(name):
    """On the reference's image alone: at most 1/4 of the values NaN, at least 1/4 finite and non-zero, and every hostile material the
    first hit of at least 4 pixels (the oracle's G-buffer ray of the pixel)."""
    g = S.golden(name)
    img = g["image"]
    nan, live = int(np.isnan(img).sum()), int((np.isfinite(img) & (img != 0)).sum())
    print(f"{name}: NaN {nan}, finite and non-zero {live} of {img.size}")
    assert 4 * nan <= img.size, (name, nan)
    assert 4 * live >= img.size, (name, live)
    d = g["desc"]
    seen = S.first_hit_pixels(d)
    hostile = [(i, k) for i, m in enumerate(d.meshes) for k in range(len(m.materials)) if S.is_hostile(m.materials[k])]
    assert hostile or name == "nan_normal", name
    for key in hostile:
        assert seen[key] >= 4, (name, key, seen[key])
    if name == "nan_normal":
        assert np.isnan(d.meshes[1].normals).any() and seen[(1, 0)] >= 4
    else:  # the patch whose shading normal faces away from its geometry (and from the sun)
        assert name in S.BOXES or ((d.meshes[1].normals == (0, 0, -1)).all() and seen[(1, 0)] >= 4)


def test_the_fixture_reaches_inf_negative_and_nan_and_the_box_goes_deep():
    imgs = np.concatenate([S.golden(n)["image"].reshape(-1) for n in S.FIXTURE])
    assert np.isinf(imgs).any() and (imgs < 0).any() and np.isnan(imgs).any()
    for name in S.BOXES:
        if name in S.FIXTURE:
            g = S.golden(name)
            d = g["desc"]
            # a path sends one ray per depth, so more than 6 rays per path on average needs paths beyond depth 5 (roulette starts past 4)
            assert g["rays"][0] - g["rays"][1] > 6 * d.width * d.height * S.SPP, (name, g["rays"])


# ----------------------------------------------------------------------------- refraction, as the product defines it
def test_refraction_scatters_a_counted_ray_that_misses():
    """A stage whose every surface is an emissive refraction material, no light: every camera path that hits sends exactly one scatter ray,
    which misses (normalize(0) is NaN), so raysTraced = camera rays + first hits at every depth cap >= 1, and the image is the emission."""
    d = S.desc("refract_first")
    for m in d.meshes:
        m.materials["reflectionType"] = 2
        m.materials["emissive"] = (1.0, 2.0, 3.0)
    d.light = None
    scene = T.OracleScene(d)
    n = d.width * d.height * S.SPP
    one, st1 = scene.render(S.SPP, max_depth=1, seed=S.SEED)
    hits = st1["raysTraced"] - n
    assert 0 < hits < n and st1["occludedTraced"] == 0
    deep, st14 = scene.render(S.SPP, max_depth=14, seed=S.SEED)
    assert st14["raysTraced"] == st1["raysTraced"] and deep.tobytes() == one.tobytes()
    assert np.isin(one[..., 0] * 8, np.arange(9)).all() and (one[..., 1] == 2 * one[..., 0]).all() and float(one.sum()) == 6.0 * hits / 8
