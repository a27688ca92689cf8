"""What prt_hip_deform_meshes computes on the device (include/prt_hip.h "geometry updates from device memory"), restated in numpy:
the incidence list (CSR) of a mesh, Mesh::calculateVertexNormals as a per-vertex walk over it (f32 throughout, the normalize / length
of vecmath.h), the bounds -> radius formula of Scene::add, and the SAH sums of prt_hip_mesh_info (math.fsum over f32 areas).  Also
hostile_mesh(): every case in which the walk can go wrong, in one small mesh."""
import math

import numpy as np

F = np.float32


def csr(indices, vertex_count):
    """(off, face): off[v]..off[v + 1] are vertex v's entries of `face`, in the order the reference's loop (faces descending, corners
    ascending within a face, mesh.cpp:112-133) reaches v's corners; a face that names v twice appears twice."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 3)
    n = len(idx)
    faces = np.repeat(np.arange(n - 1, -1, -1), 3)
    verts = idx[::-1].reshape(-1)
    order = np.argsort(verts, kind="stable")
    off = np.zeros(vertex_count + 1, dtype=np.int64)
    np.cumsum(np.bincount(verts, minlength=vertex_count), out=off[1:])
    return off, faces[order]


def _dot(a):
    return (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]


def _normalize(a):
    with np.errstate(all="ignore"):
        inv = F(1.0) / np.sqrt(_dot(a), dtype=F)
        return (inv[..., None] * a).astype(F)


def face_normals(indices, positions):
    """normalize(cross(p1 - p0, p2 - p0)) per face, (0, 0, 0) where a component is NaN."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 3)
    P = np.ascontiguousarray(positions, dtype=F).reshape(-1, 3)
    a, b = P[idx[:, 1]] - P[idx[:, 0]], P[idx[:, 2]] - P[idx[:, 0]]
    with np.errstate(all="ignore"):
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]],
                     axis=1).astype(F)
    n = _normalize(c)
    n[np.isnan(n).any(axis=1)] = 0.0
    return n


def vertex_normals(indices, positions):
    """The per-vertex walk: n = acc + fn; if (sqrtf(dot(n, n)) > 0) acc = n; over the vertex's incidence list, then normalize(acc)."""
    P = np.ascontiguousarray(positions, dtype=F).reshape(-1, 3)
    off, face = csr(indices, len(P))
    fn = face_normals(indices, P)
    acc = np.zeros((len(P), 3), F)
    valence = off[1:] - off[:-1]
    with np.errstate(all="ignore"):
        for k in range(int(valence.max()) if len(valence) else 0):
            v = np.nonzero(valence > k)[0]
            n = (acc[v] + fn[face[off[v] + k]]).astype(F)
            take = np.sqrt(_dot(n), dtype=F) > 0
            acc[v[take]] = n[take]
    return _normalize(acc)


def bits_equal(a, b):
    """bit for bit, NaN matching NaN in the same component"""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool((nan | (a.view(np.uint32) == b.view(np.uint32))).all())


def vertex_box(positions):
    """Mesh::calculateBounds: lower, upper over ALL vertices."""
    P = np.asarray(positions, dtype=F).reshape(-1, 3)
    return np.concatenate([P.min(axis=0), P.max(axis=0)]).astype(F)


def radius(boxes):
    """Scene::add (scene.cpp:23-26): boxes merged, center = 0.5f * (upper + lower), radius = length(upper - center), in f32."""
    b = np.asarray(boxes, dtype=F).reshape(-1, 6)
    lo, hi = b[:, :3].min(axis=0), b[:, 3:].max(axis=0)
    e = hi - F(0.5) * (hi + lo)
    return np.sqrt(_dot(e), dtype=F)


def box_area(lower, upper):
    """vecmath.cpp:75-79, f32"""
    e = (np.asarray(upper, dtype=F) - np.asarray(lower, dtype=F)).astype(F)
    return (F(2.0) * ((e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2]) + e[..., 2] * e[..., 0])).astype(F)


def sah(nodes):
    """dict(internalArea, leafArea, rootArea, sahCost, internalNodes, leaves, terms) of a node array (NODE_DTYPE): f32 areas, exact sums."""
    area = box_area(nodes["lower"], nodes["upper"]).astype(np.float64)
    inner = nodes["primCount"] == 0xF
    internal = math.fsum(area[inner])
    leaf = math.fsum(nodes["primCount"][~inner].astype(np.float64) * area[~inner])
    root = float(area[0])
    return dict(internalArea=internal, leafArea=leaf, rootArea=root, sahCost=(0.125 * internal + leaf) / root,
                internalNodes=int(inner.sum()), leaves=int((~inner).sum()))


def hostile_mesh():
    """(indices (faces, 3) uint32, positions (V, 3) float32) of about 700 vertices and 1100 faces:
    a regular grid patch (with -0.0 coordinates); a closed fan whose hub has valence 300 (more than one wave, more than one 256-lane
    block of corners); two coincident triangles of opposite winding on the same three vertices (the skip rule fires: n = 0); a
    triangle with two equal positions (cross = 0, normalize = NaN, set to 0) whose vertices have degenerate faces only; a face that
    names a vertex twice; a triangle so small that the cross product underflows, and one whose cross product is denormal; one
    vertex no face uses (it still counts for the bounds); counts that are no multiples of 256."""
    P, idx = [], []
    g = 20  # grid patch: g x g vertices in z = a ripple, some coordinates exactly -0.0
    for y in range(g):
        for x in range(g):
            P.append((x * 0.05 - 0.5, y * 0.05 - 0.5, 0.02 * math.sin(0.7 * x) * math.cos(0.9 * y)))
    for y in range(g - 1):
        for x in range(g - 1):
            a = y * g + x
            idx += [(a, a + 1, a + g), (a + 1, a + g + 1, a + g)]
    P = [list(p) for p in P]
    P[0][2] = -0.0
    P[10 * g + 10] = [-0.0, -0.0, P[10 * g + 10][2]]
    hub = len(P)  # fan
    P.append([1.5, 0.0, 0.3])
    rim = 300
    for k in range(rim):
        t = 2.0 * math.pi * k / rim
        P.append([1.5 + 0.4 * math.cos(t), 0.4 * math.sin(t), 0.05 * math.sin(5 * t)])
    for k in range(rim):
        idx.append((hub, hub + 1 + k, hub + 1 + (k + 1) % rim))
    c = len(P)  # coincident triangles, opposite winding
    P += [[0.0, 1.0, 0.0], [0.3, 1.0, 0.0], [0.0, 1.3, 0.1]]
    idx += [(c, c + 1, c + 2), (c, c + 2, c + 1)]
    d = len(P)  # two equal positions: these three vertices have a degenerate face only
    P += [[-1.0, 1.0, 0.2], [-1.0, 1.0, 0.2], [-0.8, 1.1, 0.2]]
    idx.append((d, d + 1, d + 2))
    idx.append((5, 5, 6))  # a grid vertex named twice
    t = len(P)  # at the origin, where small offsets are exact: the cross product (1e-46) underflows to 0
    P += [[0.0, 0.0, 0.0], [1e-23, 0.0, 0.0], [0.0, 1e-23, 0.0]]
    idx.append((t, t + 1, t + 2))
    s = len(P)  # ... and here it is denormal (1e-40): its square underflows, 1 / 0 = inf, inf * 0 = NaN
    P += [[0.0, 0.0, 0.0], [1e-20, 0.0, 0.0], [0.0, 1e-20, 0.0]]
    idx.append((s, s + 1, s + 2))
    P.append([3.0, -2.0, 4.0])  # used by no face
    P = np.array(P, dtype=F)
    idx = np.array(idx, dtype=np.uint32)
    assert len(P) % 256 and len(idx) % 256 and 650 <= len(P) <= 750 and 1000 <= len(idx) <= 1200, (len(P), len(idx))
    return idx, P
