"""InfiniteAreaLight::sample on hostile maps and draws without a GPU (tests/prt_hostile_env.py; the GPU half is
tests/test_gpu_hostile_env.py): the generator reproduces the stored inputs and labels what the reference leaves undefined; the stored
draws reach every path of the two searches (counted from the stored tables and asserted); a Python restatement of the kernels' cdf_find
-- bisection plus the `first` constant -- selects what the reference's linear scan selects on every stored draw; the oracle's tables,
its env_sample and its whole renders equal the COMPILED reference's answers in tests/golden/hostile_env.npz at tolerance 0; and the
host arithmetic of the table kernels refuses the maps that every way into the library refuses."""
import numpy as np
import pytest

import prt_amd
import prt_hostile_env as E
import prt_testlib as T
from prt_hostile_taps import words_equal_but_nan

F = np.float32
need_ref = pytest.mark.skipif(T.ref_binary("ref_path") is None, reason="oracle/_ref/ref_path is not built (no reference sources here)")
MIN_COVER = 32  # how often every path below must occur among the stored draws


@pytest.fixture(scope="module", autouse=True)
def built():
    prt_amd.build()


def named():
    return list(E.golden().items())


def host_tables(d):
    """(vertical, horizontal (h, w), firstX, firstY) of the stored texels from the host arithmetic of the table kernels."""
    v, hor, fx, fy, flags = prt_amd.env_tables_host(d["texels"])
    assert flags == 0
    return v, hor.reshape(d["texels"].shape[:2]), fx, fy


# ----------------------------------------------------------------------------- the generator and the fixture
def test_generator_reproduces_the_stored_inputs():
    z, g = E.golden(), E.generate()
    assert [n for n, _ in E.maps()] == list(z)
    for name, d in z.items():
        for field in ("texels", "u", "undefined"):
            a, b = g[f"{name}/{field}"], d[field].astype(np.uint8) if field == "undefined" else d[field]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, field)
    total = sum(len(d["u"]) for d in z.values())
    assert total <= E.MAX_DRAWS
    print("draws per map:", {n: len(d["u"]) for n, d in z.items()}, "total", total)


def test_undefined_draws_are_labelled_and_rare():
    """`undefined` is exactly "the scan over the REFERENCE's vertical table selects no row"; at most 20 % of any map with two rows or
    more, at most 5 % of all draws, every draw of the one-row map; and every draw is in [0, 1)."""
    total = undefined = 0
    for name, d in named():
        u, h = d["u"], d["texels"].shape[0]
        assert u.dtype == F and ((u >= 0) & (u < 1)).all(), name
        assert np.array_equal(E.scan(d["ref_vertical"], u[:, 1]) == h, d["undefined"]), name
        assert u[0].tolist() == [0.0, 0.0] and (u[:, 1] == E.TOP).any() and (u[:, 0] == E.TOP).any(), name
        share = d["undefined"].mean()
        print(f"{name}: {int(d['undefined'].sum())} of {len(u)} undefined ({share:.4f})")
        if h >= 2:
            assert share <= 0.20, (name, share)
            total, undefined = total + len(u), undefined + int(d["undefined"].sum())
        else:
            assert d["undefined"].all(), name
        assert not d["ref_dir"][d["undefined"]].any() and not d["ref_color"][d["undefined"]].any(), name
        assert ("ref_image" in d) == E.always_defined(d["ref_vertical"]), name
    assert undefined <= 0.05 * total, (undefined, total)
    # a map whose table ends at or below the largest draw makes the undefined case reachable by the generator: the frame tests leave it out
    assert [n for n, d in named() if "ref_image" not in d] == ["h1", "second_black"]


def test_stored_draws_reach_every_path_of_the_two_searches():
    count = dict.fromkeys(("vertical first == 1", "vertical first > 1", "horizontal first == 1", "horizontal first > 1", "u.y equals an entry",
                           "u.x equals an entry", "row ends the search (x == width)", "plateau under the selected entry (vertical)",
                           "plateau under the selected entry (horizontal)", "|theta| >= 120", "|phi| >= 120", "non-finite colour"), 0)
    for name, d in named():
        v, hor = d["ref_vertical"], d["ref_horizontal"]
        h, w = hor.shape
        _, _, fx, fy = host_tables(d)
        ok = ~d["undefined"]
        u = d["u"][ok]
        rows = E.scan(v, u[:, 1])
        with np.errstate(invalid="ignore"):
            patch_y = (h > 1) & (v[0] > u[:, 1])
            row0 = hor[rows, 0]
            patch_x = (w > 1) & (row0 > u[:, 0])
            fxr = fx[rows]
            cols = np.array([int(E.scan(hor[r], x)[0]) for r, x in zip(rows, u[:, 0])], dtype=np.int64)
            count["vertical first == 1"] += int((patch_y & (fy == 1)).sum())
            count["vertical first > 1"] += int((patch_y & (fy > 1)).sum())
            count["horizontal first == 1"] += int((patch_x & (fxr == 1)).sum())
            count["horizontal first > 1"] += int((patch_x & (fxr > 1)).sum())
            count["u.y equals an entry"] += int(np.isin(u[:, 1], v).sum())
            count["u.x equals an entry"] += int((hor[rows] == u[:, :1]).any(axis=1).sum())
            count["row ends the search (x == width)"] += int((cols == w).sum())
            # the entry two below the selected one equals the one below it: a bisection that stops one early lands on a zero pdf
            count["plateau under the selected entry (vertical)"] += int(((rows >= 2) & (v[rows - 1] == v[np.maximum(rows - 2, 0)])).sum())
            inside = cols < w
            c = np.minimum(cols, w - 1)
            count["plateau under the selected entry (horizontal)"] += int((inside & (c >= 2) & (hor[rows, c - 1] == hor[rows, np.maximum(c - 2, 0)])).sum())
        theta, phi = E.theta_phi(v, hor, u)
        count["|theta| >= 120"] += int((np.abs(theta) >= 120).sum())
        count["|phi| >= 120"] += int((np.abs(phi) >= 120).sum())
        count["non-finite colour"] += int((~np.isfinite(d["ref_color"][ok])).any(axis=1).sum())
    print("coverage:", count)
    for what, n in count.items():
        assert n >= (1 if what == "non-finite colour" else MIN_COVER), (what, n)


# ----------------------------------------------------------------------------- the search
def test_bisection_with_first_equals_the_linear_scan_on_every_stored_draw():
    """cdf_find (prt_device.h) restated in Python with the host-built `first` constants against the reference's scan over the reference's
    tables, in both dimensions; the rows of the second search are the ones the first selects, all of them where it selects none."""
    for name, d in named():
        v, hor = d["ref_vertical"], d["ref_horizontal"]
        h, w = hor.shape
        hv, hh, fx, fy = host_tables(d)
        assert hv.tobytes() == v.tobytes() and hh.tobytes() == hor.tobytes(), name  # the constants belong to these very tables
        assert fy == E.first_step(v) and fx.tolist() == [E.first_step(r) for r in hor], name
        u = d["u"]
        rows = E.scan(v, u[:, 1])
        assert np.array_equal(E.cdf_find(v, fy, u[:, 1]), rows), name
        for y in range(h):
            ux = u[rows == y, 0] if (rows == y).any() else u[:, 0]
            assert np.array_equal(E.cdf_find(hor[y], int(fx[y]), ux), E.scan(hor[y], ux)), (name, y)


# ----------------------------------------------------------------------------- the oracle
def test_oracle_tables_equal_the_compiled_references():
    for name, d in named():
        v, hor = E.tables(d["texels"])
        assert v.tobytes() == d["ref_vertical"].tobytes() and hor.tobytes() == d["ref_horizontal"].tobytes(), name


def test_oracle_env_sample_equals_the_compiled_reference_on_every_defined_draw():
    nan = 0
    for name, d in named():
        ok = ~d["undefined"]
        got = E.oracle_words(d["texels"], d["u"])
        nan += words_equal_but_nan(got[ok], E.ref_words(d)[ok], f"{name}: oracle against the compiled reference")
    print("NaN / NaN pairs with other bits:", nan)


def test_oracle_renders_equal_the_compiled_references():
    for name, d in named():
        if "ref_image" not in d:
            continue
        w, h, spp = E.RENDER
        rgb, st = T.OracleScene(E.render_desc(d["texels"])).render(spp)
        words_equal_but_nan(rgb, d["ref_image"], f"{name}: oracle render against the compiled reference")
        assert [st["raysTraced"], st["occludedTraced"]] == d["ref_rays"].tolist(), name


@need_ref
@pytest.mark.parametrize("name", ["2x2", "plateaus", "range"])
def test_the_fixture_is_what_the_compiled_reference_answers(name):
    d = E.golden()[name]
    ok = ~d["undefined"]
    vp, hp, dirs, colors = T.ref_envlight(E.render_desc(d["texels"]), d["u"][ok])
    assert vp.tobytes() == d["ref_vertical"].tobytes() and hp.tobytes() == d["ref_horizontal"].tobytes()
    words_equal_but_nan(np.concatenate([dirs, colors], axis=1), E.ref_words(d)[ok], name)


# ----------------------------------------------------------------------------- refusals
def test_host_arithmetic_refuses_the_refused_maps():
    for name, env, flags in E.refused_maps():
        assert prt_amd.env_tables_host(env)[4] == flags, name
