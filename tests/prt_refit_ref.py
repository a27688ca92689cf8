"""The refit rule of prt_hip_update_meshes / Scene.update_positions (include/prt_hip.h "geometry updates"), restated in numpy:
    leaf:      lower = min, upper = max per component over the 3 x primCount vertices of its triangles
    internal:  lower = min(child0.lower, child1.lower), upper = max(child0.upper, child1.upper)
in f32, on a node array in the reference's depth-first order (first child = i + 1, second child = primOrSecondNodeIndex > i)."""
import numpy as np

import prt_amd
import prt_testlib as T


def refit_nodes(nodes, remap, indices, positions):
    """nodes (NODE_DTYPE) with the same topology and boxes refitted to `positions` ((V, 3) float32); nothing else changes."""
    out = nodes.copy()
    P = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    corners = P[np.asarray(indices).reshape(-1, 3)[np.asarray(remap)]]  # (prims in leaf order, 3, 3)
    for i in range(len(out) - 1, -1, -1):
        n = out[i]
        if n["primCount"] == 0xF:
            a, b = out[i + 1], out[int(n["primOrSecondNodeIndex"])]
            out["lower"][i] = np.minimum(a["lower"], b["lower"])
            out["upper"][i] = np.maximum(a["upper"], b["upper"])
        else:
            k = int(n["primOrSecondNodeIndex"])
            pts = corners[k:k + int(n["primCount"])].reshape(-1, 3)
            out["lower"][i] = pts.min(axis=0)
            out["upper"][i] = pts.max(axis=0)
    return out


# the rigid moves of the teapot for which a REBUILD gives the refit's tree (tests/test_refit_cpu.py checks it; the GPU suite relies on it)
RIGID_MOVES = {
    "scale2": lambda P: (np.float32(2.0) * P).astype(np.float32),
    "scale0.5": lambda P: (np.float32(0.5) * P).astype(np.float32),
    "shift0.25x": lambda P: (P + np.array([0.25, 0.0, 0.0], dtype=np.float32)).astype(np.float32),
}


def bend(P):
    P = np.ascontiguousarray(P, dtype=np.float32)
    return (P + np.float32(0.05) * np.sin(np.float32(6.0) * P[:, [1, 2, 0]], dtype=np.float32)).astype(np.float32)


def no_negative_zero(a):
    a = np.asarray(a, dtype=np.float32)
    return not np.signbit(a[a == 0]).any()


# ----------------------------------------------------------------------------- the scenes the refit and deform tests move
def teapot_scene(size=64):
    return prt_amd.setup_cornell_box(size, size, teapot_mesh=T.teapot_product_mesh())


def atrium_scene():
    return prt_amd.setup_atrium_standin(64, 64, tris=4000, emissive_fraction=0.05)
