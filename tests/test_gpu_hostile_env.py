"""InfiniteAreaLight::sample on the MI355X (tests/prt_hostile_env.py; the CPU half is tests/test_hostile_env_cpu.py): the kernels'
env_sample / cdf_find -- bisection plus the `first` constants where the reference scans -- on the uploaded scene's own tables, through
prt_hip_test_env_sample, against the answers of the COMPILED reference stored in tests/golden/hostile_env.npz and against the live
oracle; then the frame kernel under the same maps.  Tolerance 0: the 32-bit words are equal; only a NaN may answer a NaN with other
bits."""
import ctypes as C

import numpy as np
import pytest

import prt_amd
import prt_hostile_env as E
import prt_testlib as T
from prt_gpukit import SENTINEL, TAIL, assert_same_image, sentinel, upload
from prt_gpukit import gpu_event_accounting, rows, rows2, tracer  # noqa: F401  (fixtures)
from prt_hostile_taps import words_equal_but_nan

pytestmark = pytest.mark.gpu
F = np.float32
EINVAL, ESTATE = -2, -5
NAMES = list(E.golden())
FRAME_NAMES = [n for n in NAMES if E.golden()[n]["texels"].shape[0] >= 2]
ANSWER = slice(0, 6)  # dir, color


def box_under(env):
    """(Scene, Camera, exposure): the Cornell box without the teapot at E.RENDER's size under `env`."""
    scene, camera, exposure = prt_amd.setup_cornell_box(E.RENDER[0], E.RENDER[1])
    scene.set_infinite_area_light(env)
    return scene, camera, exposure


_fresh = {}


def fresh_rows(t, name, counting):
    """The (N, 8) words of the map's stored draws on context t after a FRESH upload of the box under it: tables and `first` constants
    built on the host.  Computed once per (map, flavour)."""
    if (name, counting) not in _fresh:
        d = E.golden()[name]
        t.upload_scene(box_under(d["texels"])[0])
        _fresh[name, counting] = t.test_env_sample(d["u"], counting=counting)
    return _fresh[name, counting]


# ----------------------------------------------------------------------------- rows against the reference and the oracle
@pytest.mark.parametrize("counting", [False, True], ids=["timed", "counting"])
@pytest.mark.parametrize("name", NAMES)
def test_rows_equal_the_compiled_reference_and_the_oracle(rows, name, counting):
    d = E.golden()[name]
    got = fresh_rows(rows, name, counting)
    ok = ~d["undefined"]
    words_equal_but_nan(got[ok][:, ANSWER], E.ref_words(d)[ok], f"{name}: against the compiled reference")
    # where the reference reads past its table the kernel and the oracle share one rule (prt_device.h env_sample, prt_oracle.c env_sample)
    words_equal_but_nan(got[:, ANSWER], E.oracle_words(d["texels"], d["u"]), f"{name}: against the oracle")
    assert (got[:, 6] == (1 if counting else 0)).all() and not got[:, 7].any()


@pytest.mark.parametrize("counting", [False, True], ids=["timed", "counting"])
def test_tables_built_on_the_device_give_the_same_rows(rows, rows2, counting):
    """One context walks through every map by prt_hip_update_lights -- tables and `first` constants from the device kernels, every size
    after another one -- and answers every map's draws byte for byte as the context that uploaded it."""
    scene = box_under(E.golden()[NAMES[-1]]["texels"])[0]
    rows2.upload_scene(scene)
    for name in NAMES:
        d = E.golden()[name]
        scene.set_infinite_area_light(d["texels"])
        rows2.update_lights(scene)
        assert rows2.test_env_sample(d["u"], counting=counting).tobytes() == fresh_rows(rows, name, counting).tobytes(), name


@pytest.mark.parametrize("n,blocks", [(1, 0), (63, 0), (65, 0), (257, 1), (3000, 7)])
def test_rows_in_launches_smaller_than_a_wave_and_larger_than_a_grid_trip(rows, n, blocks):
    """1, 63 and 65 draws leave lanes idle; 257 draws on one workgroup stride twice; 3000 on 7 end a trip in the middle of a workgroup.
    The entry writes n x 8 words and nothing behind them."""
    d = E.golden()["range"]
    rows.upload_scene(box_under(d["texels"])[0])
    first = 200  # a window inside the map's draws
    u = np.ascontiguousarray(np.resize(d["u"][first:], (n, 2)))
    out = sentinel(8 * n + TAIL)
    rows._chk(rows._L.prt_hip_test_env_sample(rows._ctx, n, u.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 0, blocks),
              "prt_hip_test_env_sample")
    assert (out[8 * n:] == SENTINEL).all()
    words_equal_but_nan(out[:8 * n].reshape(n, 8)[:, ANSWER], E.oracle_words(d["texels"], u), f"n={n} blocks={blocks}")
    assert not out[:8 * n].reshape(n, 8)[:, 6:].any()


# ----------------------------------------------------------------------------- every reachable draw in one dimension
def hashed(k):
    """A fixed hash of k on the generator's grid."""
    return (((k.astype(np.uint64) * 2654435761 + 12345) & 0xffffffff) >> 9).astype(F) * E.GRID


@pytest.mark.parametrize("axis", ["u.y", "u.x"])
@pytest.mark.parametrize("name", ["plateaus", "bright_first"])
def test_every_draw_of_the_generator_in_one_dimension(rows, name, axis):
    """All 2^23 values k * 2^-23 as one coordinate, the other one hashed from k, in chunks of 2^20 against the live oracle."""
    env = E.golden()[name]["texels"]
    rows.upload_scene(box_under(env)[0])
    o = E.oracle_scene(env)
    try:
        for chunk in range(8):
            k = np.arange(chunk << 20, (chunk + 1) << 20, dtype=np.uint32)
            u = np.empty((len(k), 2), dtype=F)
            u[:, 1 if axis == "u.y" else 0] = k.astype(F) * E.GRID
            u[:, 0 if axis == "u.y" else 1] = hashed(k)
            got = rows.test_env_sample(u)[:, ANSWER]
            want = np.concatenate(o.env_sample(u), axis=1).view(np.uint32)
            bad = (got != want) & ~(np.isnan(got.view(F)) & np.isnan(want.view(F)))
            if bad.any():
                r = int(np.nonzero(bad.any(axis=1))[0][0])
                raise AssertionError(f"{name}, {axis} = k * 2^-23: first differing k = {int(k[r])}, u = {u[r].tolist()}: {got[r]} != {want[r]}")
    finally:
        o.close()


# ----------------------------------------------------------------------------- the frame kernel
@pytest.mark.parametrize("count_traffic", [False, True], ids=["timed", "counting"])
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_frame_kernel_under_the_map_equals_the_oracle_and_the_reference(tracer, name, count_traffic):
    d = E.golden()[name]
    scene, camera, exposure = box_under(d["texels"])
    upload(tracer, scene, camera)
    spp = E.RENDER[2]
    rgb = tracer.render(spp, max_depth=6, count_traffic=count_traffic)
    st = tracer.last_stats
    ref, ost = T.OracleScene(T.scene_desc_from_product(scene, camera, exposure)).render(spp, max_depth=6)
    assert_same_image(rgb, ref, f"{name}: frame against the oracle")
    assert st["raysTraced"] == ost["raysTraced"] and st["occludedTraced"] == ost["occludedTraced"] and ost["occludedTraced"] > 0, (st, ost)
    if count_traffic:
        assert st["nTap"] == ost["nTap"] > 0, (st["nTap"], ost["nTap"])
    if "ref_image" in d:  # the compiled reference's depth is its literal 14
        rgb = tracer.render(spp, count_traffic=count_traffic)
        assert_same_image(rgb, d["ref_image"], f"{name}: frame against the compiled reference")
        assert [tracer.last_stats["raysTraced"], tracer.last_stats["occludedTraced"]] == d["ref_rays"].tolist()


# ----------------------------------------------------------------------------- refusals
def test_entry_refuses_what_it_cannot_answer(rows):
    L, u, out = rows._L, np.zeros((4, 2), dtype=F), np.zeros((4, 8), dtype=np.uint32)
    pu, po = u.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    bare = prt_amd.PathTracer(test_entry_points=True)
    try:
        assert L.prt_hip_test_env_sample(bare._ctx, 4, pu, po, 0, 0) == ESTATE  # no scene
    finally:
        bare.close()
    rows.upload_scene(prt_amd.setup_cornell_box(E.RENDER[0], E.RENDER[1])[0])
    assert L.prt_hip_test_env_sample(rows._ctx, 4, pu, po, 0, 0) == ESTATE and "no environment map" in L.prt_hip_last_error().decode()
    rows.upload_scene(box_under(E.golden()["2x2"]["texels"])[0])
    assert L.prt_hip_test_env_sample(rows._ctx, 4, pu, po, 0, 0) == 0
    for args in ((rows._ctx, 0, pu, po), (rows._ctx, 4, None, po), (rows._ctx, 4, pu, None), (None, 4, pu, po)):
        assert L.prt_hip_test_env_sample(*args, 0, 0) == EINVAL, args
    for bad in (1.0, -E.GRID, np.nan, np.inf):  # no generator output: the search and the tap are bounded for [0, 1) alone
        for col in (0, 1):
            v = u.copy()
            v[2, col] = bad
            assert L.prt_hip_test_env_sample(rows._ctx, 4, v.ctypes.data_as(C.c_void_p), po, 0, 0) == EINVAL, (bad, col)


def test_refused_maps_are_refused_by_update_and_by_upload(rows):
    """prt_hip_update_lights builds a refused map's tables in buffers of their own: the scene stays as it was.  prt_hip_upload_scene has
    let go of the old scene before it reads the new one: after a refusal the context holds none, and the entry says so."""
    d = E.golden()["plateaus"]
    scene = box_under(d["texels"])[0]
    rows.upload_scene(scene)
    before, answers = rows.shading_arrays(), rows.test_env_sample(d["u"])
    for name, env, _ in E.refused_maps():
        with pytest.raises(prt_amd.PrtError, match=E.REFUSAL_MESSAGE):
            rows.update_lights(box_under(env)[0])
        now = rows.shading_arrays()
        for k, v in before.items():
            assert now[k].tobytes() == v.tobytes(), (name, k)
    assert rows.test_env_sample(d["u"]).tobytes() == answers.tobytes()
    for name, env, _ in E.refused_maps():
        with pytest.raises(prt_amd.PrtError, match=E.REFUSAL_MESSAGE):
            rows.upload_scene(box_under(env)[0])
        with pytest.raises(prt_amd.PrtError, match="upload a scene first"):
            rows.test_env_sample(d["u"])
    rows.upload_scene(scene)
    assert rows.test_env_sample(d["u"]).tobytes() == answers.tobytes()
