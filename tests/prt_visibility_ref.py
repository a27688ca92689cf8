"""The reduce of include/prt_hip.h "visibility baking" restated in numpy: reduce(points, sets, occ), float32 throughout, vectorised
over points, with the loop over k and the tree exactly as the header orders them.  The rays are those of prt_bake_ref.rays with tMax
set (rays()).  tests/test_visibility_cpu.py pins this file against its own arithmetic; tests/test_gpu_visibility.py holds the product
to it byte for byte (prt_bake_ref.same_bytes says what that means for a NaN).  Nothing here is product code."""
import numpy as np

import prt_bake_ref as BR

F = np.float32
U = np.uint32


def rays(pts, sets, max_distance):
    """(n * K,) RAY_DTYPE: the rays of prt_bake_ref.rays with tMax = max_distance."""
    r = BR.rays(pts, sets)
    r["tMax"] = F(max_distance)
    return r


def reduce(pts, sets, occ, triple=False):
    """(n, C) float32, or (n, C, 3) with triple, from the occlusion bytes occ (n * K): one wavefront per point, lane l adds the weights
    of the k = l, l + 64, ... whose byte is 0 in order, from +0, then the tree step = 32 .. 1, a_l = a_l + a_(l + step) for l < step.
    A weight whose byte is not 0 is never an operand."""
    n, K, C = len(pts), sets.K, sets.C
    open_ = np.ascontiguousarray(occ, dtype=np.uint8).reshape(n, K) == 0
    s = pts["set"]
    ok = s < sets.nSets
    w = np.zeros((n, K, C), dtype=F)
    w[ok] = sets.weights[s[ok]]
    a = np.zeros((n, 64, C), dtype=F)  # 1. a_l = +0
    with np.errstate(all="ignore"):
        for k0 in range(0, K, 64):  # 2. trip k0 / 64 of every lane that still has a k
            m = min(64, K - k0)
            a[:, :m] = np.where(open_[:, k0:k0 + m, None], a[:, :m] + w[:, k0:k0 + m], a[:, :m])
        step = 32
        while step >= 1:  # 3.
            a[:, :step] = a[:, :step] + a[:, step:2 * step]
            step //= 2
    out = a[:, 0].copy()  # 4.
    out[~ok] = F(0.0)
    assert out.dtype == F
    return np.repeat(out[:, :, None], 3, axis=2) if triple else out
