"""The inputs the lightmap-filter tests share (tests/test_atlas_filter_cpu.py, tests/test_gpu_atlas_filter.py; a library module, no
tests of its own): the 40 x 24 atlas of two charts, the hostile points, and the file format of tests/atlas_filter_main.cpp.

The two-chart atlas.  A floor (N = +z, columns 0 .. 18) and a wall (N = +x, columns 19 .. 39) that are adjacent in the atlas and meet
at a right angle in the world, one texel = 0.1 units.  The floor has a 5 x 5 hole of unowned texels (columns 6 .. 10, rows 8 .. 12)
and the wall's last column is unowned in the odd rows.  Texels ascend, as the rasteriser gives them: rows of 40 points are shorter
than a wave, so points cross wave boundaries, and the step-16 taps of the fifth iteration leave the image on every side.  Two
adjacent floor texels share one position (d2 == 0: no footprint, wp = 1).

Hostile points.  A point that is not PLACED is never a tap, so the others' results equal those of a run without it whatever it
holds: those cases spoil an interior floor point (or append points), and the run without deletes it.  A hostile point that IS placed
can leave the others' results unchanged only where the definition gives it no say: it sits at the centre of the hole, where it has
no 8-neighbour (so it is in nobody's footprint and nobody's 3 x 3 variance average) and is a tap of the points around the hole from
step 2 on, and its geometric weight is exactly 0 (wn = 0 or wp = 0): adding w = 0 changes no sum.  `long_normal` has a weight
that is not 0 and is held to the restatement alone."""
import numpy as np

F = np.float32
U = np.uint32
POINT_DTYPE = np.dtype([("P", "<f4", 3), ("bias", "<f4"), ("N", "<f4", 3), ("set", "<u4")])
W2, H2 = 40, 24
HOLE = (6, 8, 11, 13)      # x0, y0, x1, y1 (exclusive)
HOLE_CENTRE = 10 * W2 + 8  # texel (8, 10)
SPOILT = 5 * W2 + 3        # an interior floor texel: texel (3, 5)


def two_charts(C=1, seed=3, noise=0.25, floor=None, wall=None):
    """(texels (n,), points (n,), values (n, 3*C), clean (n, 3*C), chart (n,) 0 = floor 1 = wall): a smooth signal under
    multiplicative noise; floor / wall: constants instead."""
    rng = np.random.default_rng(seed)
    own = np.ones((H2, W2), bool)
    own[HOLE[1]:HOLE[3], HOLE[0]:HOLE[2]] = False
    own[1::2, W2 - 1] = False
    t = np.nonzero(own.reshape(-1))[0].astype(U)
    x, y = (t % W2).astype(np.float64), (t // W2).astype(np.float64)
    is_wall = x >= 19
    pts = np.zeros(len(t), POINT_DTYPE)
    pts["P"][:, 0] = np.where(is_wall, 1.9, 0.1 * x)
    pts["P"][:, 1] = 0.1 * y
    pts["P"][:, 2] = np.where(is_wall, 0.1 * (x - 19) + 0.05, 0.0)
    pts["N"][:, 0] = is_wall
    pts["N"][:, 2] = ~is_wall
    pts["bias"] = 1e-3
    pts["set"] = (t % 2) + 2 * ((t // W2) % 2)
    twin = np.nonzero(t == 15 * W2 + 4)[0][0]
    pts["P"][twin] = pts["P"][twin - 1]  # texels (3, 15) and (4, 15) at one position
    ch = np.arange(3 * C, dtype=np.float64)[None, :]
    clean = (1.0 + 0.5 * np.sin(0.08 * x[:, None] + 0.2 * ch) * np.cos(0.07 * y)[:, None] + 0.1 * ch) * np.where(is_wall, 2.5, 1.0)[:, None]
    if floor is not None:
        clean = np.where(is_wall[:, None], wall, floor) + 0.0 * clean
    values = clean * (1.0 + noise * rng.normal(size=clean.shape)) if noise else clean
    return t, pts, values.astype(F), clean.astype(F), is_wall.astype(np.int64)


def _delete(k, *arrays):
    return tuple(np.delete(a, k, axis=0) for a in arrays)


def _append(t, pts, v, texel, P=None, N=None, values=None, set_=0, like=0):
    p = pts[like:like + 1].copy()
    if P is not None:
        p["P"][0] = P
    if N is not None:
        p["N"][0] = N
    p["set"] = set_
    row = v[like:like + 1].copy() if values is None else np.asarray(values, F).reshape(1, -1)
    return np.concatenate([t, np.array([texel], U)]), np.concatenate([pts, p]), np.concatenate([v, row])


HOSTILE = ("duplicate", "texel_outside", "never_set", "nan_c0", "inf_c0", "nan_later", "inf_later", "nan_P", "nan_N", "inf_P",
           "zero_normal", "tiny_normal", "opposed_normal", "same_position", "isolated", "far_1e30")
REF_ONLY = ("long_normal", "huge_values")  # held to the restatement alone


def hostile(kind, C=2):
    """((texels, points, values) with the hostile points, the same without them or None, `keep`: the indices of the first whose
    results the second must reproduce, in the second's order)."""
    t, pts, v, _, _ = two_charts(C=C, seed=11)
    n = len(t)
    k = int(np.nonzero(t == SPOILT)[0][0])
    base = (t, pts, v)
    others = np.delete(np.arange(n), k)
    if kind == "duplicate":  # three points on one texel: the first is not eligible, the second is placed, the third is not
        v2 = v.copy()
        v2[k, 0] = np.nan
        a = _append(t, pts, v2, SPOILT, values=v[k] * F(3.0), like=k)
        a = _append(*a, SPOILT, values=v[k] * F(0.5), like=k)
        wo = _delete(k, *_append(t, pts, v, SPOILT, values=v[k] * F(3.0), like=k))
        return a, wo, np.delete(np.arange(n + 1), k)
    if kind == "texel_outside":
        a = _append(t, pts, v, W2 * H2)
        a = _append(*a, 0xffffffff)
        return a, base, np.arange(n)
    spoil = {"never_set": ("set", None), "nan_c0": ("v", (1, np.nan)), "inf_c0": ("v", (0, np.inf)), "nan_later": ("v", (3 * C - 1, np.nan)),
             "inf_later": ("v", (3, -np.inf)), "nan_P": ("P", (1, np.nan)), "nan_N": ("N", (2, np.nan)), "inf_P": ("P", (0, np.inf))}
    if kind in spoil:
        field, how = spoil[kind]
        pts2, v2 = pts.copy(), v.copy()
        if field == "set":
            pts2["set"][k] = 0xffffffff
        elif field == "v":
            v2[k, how[0]] = how[1]
        else:
            pts2[field][k, how[0]] = how[1]
        return (t, pts2, v2), _delete(k, t, pts, v), others
    centre = {"zero_normal": dict(N=(0, 0, 0)), "tiny_normal": dict(N=(0, 0, 1e-30)), "opposed_normal": dict(N=(0, 0, -1)),
              "isolated": dict(P=(900.0, -700.0, 40.0)), "far_1e30": dict(P=(1e30, 0.5, -1e30)), "long_normal": dict(N=(0, 0, 3))}
    if kind in centre:  # at the centre of the hole, where the floor would be
        a = _append(t, pts, v, HOLE_CENTRE, **dict(dict(P=(0.8, 1.0, 0.0)), **centre[kind]))
        return a, (None if kind in REF_ONLY else base), np.arange(n)
    if kind == "same_position":  # the other side of a thin floor: the position of texel (4, 10), a tap at steps 2 and 4, the normal reversed
        q = int(np.nonzero(t == 10 * W2 + 4)[0][0])
        a = _append(t, pts, v, HOLE_CENTRE, P=pts["P"][q], N=(0, 0, -1))
        return a, base, np.arange(n)
    if kind == "huge_values":
        return (t, pts, (v * (F(2e38) / v.max())).astype(F)), None, np.arange(n)  # finite: the squares and the sums overflow
    raise KeyError(kind)


def owned(W, H, C=1, seed=5):
    """A fully owned W x H atlas on one plane: the 129 x 5, 1 x 1 and beyond-one-trip cases."""
    rng = np.random.default_rng(seed)
    t = np.arange(W * H, dtype=U)
    pts = np.zeros(W * H, POINT_DTYPE)
    pts["P"][:, 0], pts["P"][:, 1] = 0.25 * (t % W), 0.25 * (t // W)
    pts["N"][:, 2] = 1.0
    v = (1.0 + 0.3 * rng.random((W * H, 3 * C))).astype(F)
    return t, pts, v


# ----------------------------------------------------------------------------- tests/atlas_filter_main.cpp
def write_cases(path, cases):
    """cases: [(W, H, texels, points, values, iterations, npl2, sigma_l, sigma_p)]."""
    with open(path, "wb") as fh:
        fh.write(np.array([len(cases)], U).tobytes())
        for W, H, t, pts, v, it, npl2, sl, sp in cases:
            v = np.ascontiguousarray(v, F).reshape(len(t), -1)
            fh.write(np.array([W, H, len(t), v.shape[1], it, npl2], U).tobytes() + np.array([sl, sp], F).tobytes())
            fh.write(np.ascontiguousarray(t, U).tobytes() + np.ascontiguousarray(pts).tobytes() + v.tobytes())


def read_results(path, cases):
    words = np.fromfile(path, dtype=U)
    out, at = [], 0
    for W, H, t, pts, v, *_ in cases:
        size = np.asarray(v).size
        out.append(words[at:at + size].reshape(len(t), -1))
        at += size
    assert at == len(words), (at, len(words))
    return out
