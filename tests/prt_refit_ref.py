"""The refit rule of prt_hip_update_meshes / Scene.update_positions (include/prt_hip.h "geometry updates"), restated in numpy:
    leaf:      lower = min, upper = max per component over the 3 x primCount vertices of its triangles
    internal:  lower = min(child0.lower, child1.lower), upper = max(child0.upper, child1.upper)
in f32, on a node array in the reference's depth-first order (first child = i + 1, second child = primOrSecondNodeIndex > i)."""
import numpy as np


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
