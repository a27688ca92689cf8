"""Rows a12 / a14 on the MI355X (tests/prt_hostile_taps.py; the CPU half is tests/test_hostile_taps_cpu.py): the kernels' texture taps
(tex_sample3, tex_sample1, sample_diffuse, the alpha decision of a leaf round in both flavours -- class word first, then the blend) and
their surface fetch (get_surface, sample_bump) on the uploaded scene's own arrays, through prt_hip_test_taps / prt_hip_test_surface,
against the answers of the COMPILED reference's texture.cpp / material.cpp / mesh.cpp stored in tests/golden/hostile_taps.npz.
Tolerance 0: the 32-bit words are equal; only a NaN may answer a NaN with other bits (degenerate triangles)."""
import numpy as np
import pytest

import prt_amd
import prt_hostile_taps as H
import prt_testlib as T
from prt_gpukit import assert_bits_equal, snapped_scene

pytestmark = pytest.mark.gpu
F = np.float32
TAP_WORDS = slice(0, 9)      # sample3, sample1, alpha single, alpha packet, sampleDiffuse
SURFACE_WORDS = slice(0, 19)  # normal, uv, material, duv01, duv02, dp01, dp02, sampleBump's normal


# (differs from prt_gpukit.rows: the golden scene is uploaded, and the fixture is (context, golden arrays))
@pytest.fixture(scope="module")
def rows():
    prt_amd.build()
    t = prt_amd.PathTracer(test_entry_points=True)
    z = H.golden()
    t._taps_keep = H.upload(t, H.golden_desc(z))
    yield t, z
    t.close()


@pytest.mark.parametrize("counting", [False, True], ids=["timed", "counting"])
def test_taps_equal_the_compiled_reference(rows, counting):
    t, z = rows
    got = t.test_taps(z["taps"], counting=counting)
    assert H.words_equal_but_nan(got[:, TAP_WORDS], z["ref_taps"][:, TAP_WORDS], "taps") == 0
    # sample3 + sample1 + sampleDiffuse's own tap; the alpha decision of a leaf round is never counted here (the walk counts it)
    assert (got[:, 9] == (3 * (z["taps"][:, 3] & 1) if counting else 0)).all() and not got[:, 10:].any()


@pytest.mark.parametrize("n,blocks", [(5, 0), (63, 0), (257, 1), (11008, 2), (3000, 7)])
def test_taps_in_launches_smaller_than_a_wave_and_larger_than_a_grid_trip(rows, n, blocks):
    """5 and 63 records leave lanes of the one wave idle; 257 records on one workgroup and 11008 on two stride over the records 2 and 22
    times; 3000 on 7 end a trip in the middle of a workgroup."""
    t, z = rows
    first = int(z["taps_first"][10])  # a window that starts inside the big maps' records
    rec = z["taps"][:n] if n > 5000 else z["taps"][first:first + n]
    want = z["ref_taps"][:n] if n > 5000 else z["ref_taps"][first:first + n]
    assert len(rec) == n
    got = t.test_taps(rec, blocks=blocks)
    assert H.words_equal_but_nan(got[:, TAP_WORDS], want[:, TAP_WORDS], f"taps n={n} blocks={blocks}") == 0


@pytest.mark.parametrize("counting", [False, True], ids=["timed", "counting"])
def test_surface_fetch_and_bump_equal_the_compiled_reference(rows, counting):
    t, z = rows
    got = t.test_surface(z["surface"], counting=counting)
    nan = H.words_equal_but_nan(got[:, SURFACE_WORDS], z["ref_surface"][:, SURFACE_WORDS], "surface")
    deg = H.degenerate_mask(z["surface"])
    assert not np.isnan(np.delete(got[~deg][:, SURFACE_WORDS].view(F), 5, axis=1)).any(), "a NaN outside the degenerate triangles"
    print("NaN / NaN pairs with other bits:", nan)
    desc = H.golden_desc(z)
    bumped = np.array([desc.meshes[m].materials[desc.meshes[m].prim_material[p]]["bumpMap"] >= 0 for m, p in z["surface"][:, :2]])
    assert (got[:, 19] == (3 * bumped if counting else 0)).all()


@pytest.mark.parametrize("n,blocks", [(7, 0), (300, 1), (1044, 3)])
def test_surface_in_launches_smaller_than_a_wave_and_larger_than_a_grid_trip(rows, n, blocks):
    t, z = rows
    got = t.test_surface(z["surface"][-n:], blocks=blocks)
    H.words_equal_but_nan(got[:, SURFACE_WORDS], z["ref_surface"][-n:][:, SURFACE_WORDS], f"surface n={n} blocks={blocks}")


def test_entries_refuse_what_would_read_outside_the_scene(rows):
    t, z = rows
    n_mats = sum(len(m.materials) for m in H.golden_desc(z).meshes)
    grey = int(np.nonzero([tex.shape[2] == 1 for _, tex in H.golden_maps(z)])[0][0])
    for rec in ([n_mats, 0, 0, 1], [0, 0, 0, 4], [grey, 0, 0, 2], [n_mats - 3, 0, 0, 1]):  # no such material; bad flags; alpha on a grey map; no maps
        with pytest.raises(prt_amd.PrtError):
            t.test_taps(np.array([rec], dtype=np.uint32))
    for rec in ([4, 0, 0, 0, 0], [1, 20, 0, 0, 0]):
        with pytest.raises(prt_amd.PrtError):
            t.test_surface(np.array([rec], dtype=np.uint32))


@pytest.mark.parametrize("count_traffic", [False, True], ids=["timed", "counting"])
def test_render_with_uv_snapped_to_texel_edges_matches_oracle(count_traffic):
    """64 x 48, 8 spp (one packet of samples per pixel): camera rays and shadow rays through the alpha mask, diffuse taps and bump taps on quads whose texcoords lie on
    texel edges, against the oracle as usual."""
    prt_amd.build()
    desc = snapped_scene(H.golden())
    t = prt_amd.PathTracer()
    try:
        keep = H.upload(t, desc)
        t.set_camera(prt_amd.Camera().create(desc.cam_pos, desc.cam_dir, desc.width, desc.height))
        rgb = t.render(8, count_traffic=count_traffic)
        ref, ost = T.OracleScene(desc).render(8)
        assert_bits_equal(rgb, ref, "snapped uv render")
        assert t.last_stats["raysTraced"] == ost["raysTraced"] and t.last_stats["occludedTraced"] == ost["occludedTraced"]
        assert float(ref.sum()) > 0.0 and ost["nTap"] > 10000
        del keep
    finally:
        t.close()
