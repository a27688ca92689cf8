"""Lightmap atlases without a GPU (include/prt_hip.h "lightmap atlases"; the GPU half is tests/test_gpu_atlas.py): the three entry points
are declared, documented and exported, and the numpy restatement the GPU tests hold the product to (tests/prt_atlas_ref.py) is pinned
against cases worked by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import prt_amd
import prt_atlas_ref as AR
import prt_testlib as T

F = np.float32
U = np.uint32
NAMES = ("prt_hip_atlas_rasterize", "prt_hip_atlas_points", "prt_hip_atlas_resolve")


# ----------------------------------------------------------------------------- the interface
def test_header_declares_the_entry_points_and_carries_the_rules():
    src = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    assert src.index("---- baking") < src.index("---- lightmap atlases"), "the section follows the baking section"
    section = src[src.index("---- lightmap atlases"):]
    flat = re.sub(r"\s+", " ", section)
    for decl in ("typedef struct { uint32_t meshId; uint32_t primCount; const float* uv; /* 6*primCount: (u,v) of corners 0,1,2, mesh order */ } "
                 "prt_atlas_mesh;",
                 "typedef struct { uint32_t n; uint32_t rejected; uint32_t degenerate; uint32_t reserved; uint64_t pairs; } prt_atlas_counts;",
                 "typedef struct { float bias; uint32_t setTile; uint32_t reserved[2]; } prt_atlas_point_params;",
                 "int prt_hip_atlas_rasterize(prt_hip_ctx* ctx, uint32_t W, uint32_t H, uint32_t count, const prt_atlas_mesh* meshes, "
                 "uint32_t* texels /* capacity W*H */, prt_hit* hits /* capacity W*H */, prt_atlas_counts* counts /* HOST */, uint32_t flags, "
                 "void* stream);",
                 "int prt_hip_atlas_points(prt_hip_ctx* ctx, uint32_t n, uint32_t W, const uint32_t* texels, const prt_hit* hits, "
                 "const prt_atlas_point_params* params, prt_bake_point* points, uint32_t flags, void* stream);",
                 "int prt_hip_atlas_resolve(prt_hip_ctx* ctx, uint32_t W, uint32_t H, uint32_t n, const uint32_t* texels, "
                 "const float* values /* n*stride */, uint32_t stride /* 1 .. 48: 3*C of the bake */, uint32_t gutter /* 0 .. 64 */, "
                 "float* image /* W*H*stride */, uint8_t* mask /* W*H, may be NULL */, uint32_t flags, void* stream);"):
        assert decl in flat, decl
    text = re.sub(r"[\s*]+", " ", section)  # (comment stars and line breaks go; so does every '*' of a formula)
    for rule in ("fx = u (float)(256 W) (one f32 product), X = rint(fx) (ties to even)",  # snap
                 "!(fabsf(fx) <= 8388608.0f)", "counts in `rejected`",
                 "E(a,b,c) = (b.x-a.x) (c.y-a.y) - (b.y-a.y) (c.x-a.x)", "A = E(v0,v1,v2)", "a triangle with A == 0 counts in `degenerate`",
                 "c = (256x+128, 256y+128): w0 = E(v1,v2,c), w1 = E(v2,v0,c), w2 = E(v0,v1,c)", "If A < 0, negate all four",
                 "iff w0 >= 0 && w1 >= 0 && w2 >= 0", "w0+w1+w2 == A exactly", "counts in `pairs`",
                 "smallest key (meshId << 28) | primId among its covering triangles",
                 "texels[0..n) are their indices y W + x in ascending order",
                 "{t = 0, i = (float)w0/(float)A, j = (float)w1/(float)A, k = (float)w2/(float)A, primId, meshId}",
                 "Entries at and beyond n are untouched",
                 "W, H: 1 .. 8192", "count: 1 .. PRT_HIP_MAX_BVH", "each at most once", "primCount 1 .. 2^28",
                 "counts is HOST memory and the call returns when it is filled",
                 "P = (i p0 + j p1) + k p2 per component",  # points
                 "set = (x % setTile) + setTile (y % setTile) with x = texel % W, y = texel / W; setTile 1 .. 32",
                 "all-zero point with set = 0xffffffff", "meshId < the scene's mesh count, primId < that mesh's primitive count",
                 "why the atlas stores barycentrics and not positions", "PRT_HIP_ESTATE without one",
                 "Every texel starts at +0 with mask 0",  # resolve
                 "an index at or beyond W H is ignored",
                 "mask in 1 .. g takes, per float, the sum over those neighbours in the order dy = -1, 0, 1 outer, dx = -1, 0, 1 inner",
                 "divided by (float)count", "its mask becomes g + 1", "Texels filled in pass g are not read in pass g",
                 "stride: 1 .. 48", "gutter: 0 .. 64", "mask may be NULL",
                 "Other flag bits are refused", "before anything is queued and with the outputs untouched", "reserved != 0",
                 "conservative rasterisation", "seam stitching", "a count of invalid records in atlas_points"):
        assert rule in text, rule


def test_the_entry_points_are_exported_and_wrapped():
    prt_amd.build()
    for name in NAMES:
        assert name in prt_amd.EXPORTS
    for path in (prt_amd.LIB_PATH, prt_amd.TEST_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in NAMES:
            assert f" T {name}\n" in syms, (path, name)
    assert "prt_atlas.hip" in prt_amd._build.SOURCES
    for method in ("atlas_rasterize", "atlas_rasterize_device", "atlas_points", "atlas_points_async", "atlas_resolve", "atlas_resolve_async",
                   "lightmap"):
        assert callable(getattr(prt_amd.PathTracer, method))
    M, K, P = prt_amd.AtlasMesh, prt_amd.AtlasCounts, prt_amd.AtlasPointParams
    assert (C.sizeof(M), M.meshId.offset, M.primCount.offset, M.uv.offset) == (16, 0, 4, 8)
    assert (C.sizeof(K), K.n.offset, K.rejected.offset, K.degenerate.offset, K.reserved.offset, K.pairs.offset) == (24, 0, 4, 8, 12, 16)
    assert (C.sizeof(P), P.bias.offset, P.setTile.offset, P.reserved.offset) == (16, 0, 4, 8)
    assert prt_amd.HIT_DTYPE == AR.HIT_DTYPE and prt_amd.BAKE_POINT_DTYPE == AR.POINT_DTYPE


def test_the_calls_fail_loudly_without_a_context():
    """As the queries and the baker: PRT_HIP_ENODEVICE where no device exists, PRT_HIP_EINVAL for a NULL context where one does."""
    prt_amd.build()
    L = prt_amd.lib()
    want = -1 if L.prt_hip_device_count() == 0 else -2
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    mesh = prt_amd.AtlasMesh(meshId=0, primCount=1, uv=buf.ctypes.data)
    counts = prt_amd.AtlasCounts()
    params = prt_amd.AtlasPointParams(bias=0.0, setTile=1)
    assert L.prt_hip_atlas_rasterize(None, 1, 1, 1, C.byref(mesh), p, p, C.byref(counts), prt_amd.QUERY_HOST, None) == want
    assert L.prt_hip_atlas_points(None, 1, 1, p, p, C.byref(params), p, prt_amd.QUERY_HOST, None) == want
    assert L.prt_hip_atlas_resolve(None, 1, 1, 1, p, p, 1, 0, p, p, prt_amd.QUERY_HOST, None) == want
    assert L.prt_hip_last_error()
    assert not buf.any() and counts.n == 0


# ----------------------------------------------------------------------------- the restatement: rasterize
SQUARE = np.array([[[0, 0], [0.5, 0], [0.5, 0.5]], [[0, 0], [0.5, 0.5], [0, 0.5]]], F)  # prims 0 and 1 share the diagonal


def test_the_unit_square_split_along_its_diagonal():
    texels, hits, counts = AR.rasterize({0: SQUARE}, 64, 64)
    assert counts == dict(n=1024, rejected=0, degenerate=0, pairs=1056)
    x, y = texels % 64, texels // 64
    want = (np.arange(32)[:, None] * 64 + np.arange(32)[None, :]).reshape(-1)
    assert texels.dtype == U and texels.tolist() == want.tolist(), "no texel inside the square is unowned, none outside is owned"
    diagonal = x == y
    assert diagonal.sum() == 32 and (hits["primId"][diagonal] == 0).all(), "the contested centres belong to prim 0"
    assert (hits["primId"][x > y] == 0).all() and (hits["primId"][x < y] == 1).all() and not hits["meshId"].any() and not hits["t"].any()
    total = hits["i"].astype(np.float64) + hits["j"] + hits["k"]
    assert np.abs(total - 1).max() <= 2.0 ** -22
    assert (hits["i"] >= 0).all() and (hits["j"] >= 0).all() and (hits["k"] >= 0).all()
    # texel (3, 1) of prim 0 by hand: c = (896, 384), corners (0,0) (8192,0) (8192,8192), A = 8192^2
    q = int(np.nonzero(texels == 1 * 64 + 3)[0][0])
    A = 8192 * 8192
    w0, w1, w2 = (8192 - 896) * 8192, 8192 * (896 - 384), 8192 * 384
    assert w0 + w1 + w2 == A
    assert (hits["i"][q], hits["j"][q], hits["k"][q]) == (F(w0) / F(A), F(w1) / F(A), F(w2) / F(A))


def test_the_mirrored_square_gives_the_same_texels():
    mirrored = SQUARE[:, [0, 2, 1]]  # A < 0
    a, b = AR.rasterize({0: SQUARE}, 64, 64), AR.rasterize({0: mirrored}, 64, 64)
    assert a[0].tolist() == b[0].tolist() and a[2] == b[2]
    assert (a[1]["primId"] == b[1]["primId"]).all()
    assert a[1]["i"].tobytes() == b[1]["i"].tobytes() and a[1]["j"].tobytes() == b[1]["k"].tobytes(), "corners 1 and 2 change places"


def test_a_corner_exactly_on_a_texel_centre_is_covered():
    c = (F(2.5) / F(8), F(1.5) / F(8))  # the centre of texel (2, 1) of an 8 x 8 atlas, exact in float32
    tri = np.array([[c, (1.0, c[1]), (1.0, 1.0)]], F)
    texels, hits, _ = AR.rasterize({0: tri}, 8, 8)
    assert 1 * 8 + 2 in texels.tolist()
    q = texels.tolist().index(1 * 8 + 2)
    assert (hits["i"][q], hits["j"][q], hits["k"][q]) == (1.0, 0.0, 0.0)


def test_a_sliver_thinner_than_a_texel_that_crosses_no_centre_covers_nothing():
    sliver = np.array([[(0.01, 0.26), (0.99, 0.30), (0.99, 0.31)]], F)  # between the centre rows v = 0.1875 and 0.3125 of an 8 x 8 atlas
    texels, _, counts = AR.rasterize({0: sliver}, 8, 8)
    assert len(texels) == 0 and counts == dict(n=0, rejected=0, degenerate=0, pairs=0)


def test_a_tie_of_rint_snaps_to_the_even_integer():
    W = 4  # fx = u * 1024: u = 2.5 / 1024 and 3.5 / 1024 are exact, fx = 2.5 and 3.5
    uv = np.array([[(2.5 / 1024, 3.5 / 1024), (0.5 / 1024, -0.5 / 1024), (-1.5 / 1024, 1.0)]], F)
    X, Y, ok = AR.snap(uv, W, W)
    assert ok.all() and X.tolist() == [[2, 0, -2]] and Y.tolist() == [[4, 0, 1024]]


def test_rejected_and_degenerate_triangles_are_counted_and_cover_nothing():
    edge_u = F(8388608.0) / F(256 * 64)  # fabsf(fx) exactly 2^23: accepted
    tris = np.array([
        [(np.nan, 0), (1, 0), (1, 1)], [(0, 0), (np.inf, 0), (1, 1)], [(0, 0), (1, 0), (1e9, 1)],  # rejected
        [(0, 0), (1, 0), (np.nextafter(edge_u, F(np.inf)), 1)], [(0, 0), (1, 0), (1, -np.nextafter(edge_u, F(np.inf)))],  # rejected
        [(0, 0), (0.5, 0.5), (1, 1)], [(0.25, 0.25), (0.25, 0.25), (0.25, 0.25)],  # A == 0
        [(0, 0), (edge_u, 0), (0, 0.25)],  # accepted
    ], F)
    texels, _, counts = AR.rasterize({3: tris}, 64, 64)
    assert (counts["rejected"], counts["degenerate"]) == (5, 2) and counts["n"] == len(texels) > 0


# ----------------------------------------------------------------------------- the restatement: points and resolve
def test_points_follow_the_formulas_and_never_an_outside_hit():
    idx = np.array([[0, 1, 2], [2, 1, 3]], U)
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [1, 2, 5]], F)
    hits = np.zeros(4, AR.HIT_DTYPE)
    hits["i"], hits["j"], hits["k"] = [0.25, 0.5, 1, 1], [0.25, 0.25, 0, 0], [0.5, 0.25, 0, 0]
    hits["primId"], hits["meshId"] = [0, 1, 2, 0], [0, 0, 0, 1]
    N = np.array([[0, 0, 1]] * 4, F)
    pts = AR.points(np.array([0, 5 * 7 + 6, 1, 2], U), hits, 7, [(idx, pos)], N, 0.125, 4)
    assert pts["P"][0].tolist() == [0.25, 1.0, 0.0] and pts["P"][1].tolist() == [0.5, 1.5, 1.25]
    assert pts["set"].tolist() == [0, (6 % 4) + 4 * (5 % 4), AR.NEVER, AR.NEVER] and pts["bias"][:2].tolist() == [0.125, 0.125]
    assert not pts[2:]["P"].any() and not pts[2:]["N"].any() and not pts[2:]["bias"].any()


def test_gutter_fill_of_one_texel_in_a_5_by_5_image():
    """The centre holds (8, -0.0).  Pass 1 gives its eight neighbours the value over one neighbour, 8 / 1 and +0 (the sum starts
    from +0: +0 + -0 = +0); pass 2 gives the outer ring the mean of its pass-1 neighbours -- 8 again, from one (corners), two (next to
    a corner) or three (edge middles) of them."""
    image, mask = AR.resolve(np.array([12], U), np.array([[8.0, -0.0]], F), 5, 5, 2)
    assert mask.reshape(5, 5).tolist() == [[3, 3, 3, 3, 3], [3, 2, 2, 2, 3], [3, 2, 1, 2, 3], [3, 2, 2, 2, 3], [3, 3, 3, 3, 3]]
    assert (image[:, 0] == 8).all()
    bits = image[:, 1].view(U)
    assert bits[12] == 0x80000000 and not np.delete(bits, 12).any(), "the value travels as given; every fill is +0"
    one, m1 = AR.resolve(np.array([12], U), np.array([[8.0, -0.0]], F), 5, 5, 1)
    assert m1.reshape(5, 5)[0].tolist() == [0] * 5 and not one.reshape(5, 5, 2)[0].view(U).any()
    # the neighbour order shows where the sum is not associative: three sources left of a hole, summed dy = -1, 0, 1
    v = np.array([[1e8], [1.0], [-1e8]], F)
    img, mk = AR.resolve(np.array([0, 3, 6], U), v, 3, 3, 1)
    assert mk.tolist() == [1, 2, 0, 1, 2, 0, 1, 2, 0]
    assert img[4, 0] == ((F(0) + F(1e8)) + F(1.0) + F(-1e8)) / F(3) == 0.0, "1e8 + 1 rounds to 1e8"
    assert img[1, 0] == (F(1e8) + F(1.0)) / F(2) and img[7, 0] == (F(1.0) + F(-1e8)) / F(2)


def test_resolve_ignores_indices_outside_the_image_and_carries_nan():
    v = np.array([[np.nan], [2.0], [3.0], [np.inf]], F)
    img, mk = AR.resolve(np.array([0, 6, 0xffffffff, 2], U), v, 3, 2, 1)
    assert mk.tolist() == [1, 2, 1, 2, 2, 2]
    assert np.isnan(img[0, 0]) and np.isnan(img[1, 0]) and np.isnan(img[3, 0]) and np.isnan(img[4, 0])
    assert img[5, 0] == np.inf and img[2, 0] == np.inf
