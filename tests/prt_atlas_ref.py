"""The three definitions of include/prt_hip.h "lightmap atlases" restated in numpy: rasterize (int64 edge functions on np.rint-snapped
corners, ownership by the smallest key), points (float32, every product rounded before the sums) and resolve (the gutter passes in the
header's neighbour order).  tests/test_atlas_cpu.py pins this file against cases worked by hand; tests/test_gpu_atlas.py holds the
product to it byte for byte (NaN for NaN: prt_bake_ref.same_bytes).  Nothing here is product code."""
import numpy as np

F = np.float32
U = np.uint32
I = np.int64
HIT_DTYPE = np.dtype([("t", "<f4"), ("i", "<f4"), ("j", "<f4"), ("k", "<f4"), ("primId", "<u4"), ("meshId", "<u4")])
POINT_DTYPE = np.dtype([("P", "<f4", 3), ("bias", "<f4"), ("N", "<f4", 3), ("set", "<u4")])
NO_OWNER = 0xffffffff
SNAP_LIMIT = F(8388608.0)
NEVER = 0xffffffff  # the set of the point prt_hip_bake never follows


def snap(uv, W, H):
    """uv (P, 3, 2) float32 -> (X, Y (P, 3) int64, ok (P,)): ok is false where a corner's product is beyond 2^23 or a NaN."""
    uv = np.asarray(uv, dtype=F).reshape(-1, 3, 2)
    with np.errstate(all="ignore"):
        fx, fy = uv[:, :, 0] * F(256 * W), uv[:, :, 1] * F(256 * H)
        assert fx.dtype == F and fy.dtype == F
        ok = ((np.abs(fx) <= SNAP_LIMIT) & (np.abs(fy) <= SNAP_LIMIT)).all(axis=1)
        X = np.where(ok[:, None], np.rint(fx), 0).astype(I)  # (ties to even)
        Y = np.where(ok[:, None], np.rint(fy), 0).astype(I)
    return X, Y, ok


def edge(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def weights(X, Y, cx, cy):
    """(A, w0, w1, w2) of triangles X, Y (..., 3) at centres (cx, cy), the sign of A taken out of all four."""
    A = edge(X[..., 0], Y[..., 0], X[..., 1], Y[..., 1], X[..., 2], Y[..., 2])
    w0 = edge(X[..., 1], Y[..., 1], X[..., 2], Y[..., 2], cx, cy)
    w1 = edge(X[..., 2], Y[..., 2], X[..., 0], Y[..., 0], cx, cy)
    w2 = edge(X[..., 0], Y[..., 0], X[..., 1], Y[..., 1], cx, cy)
    s = np.where(A < 0, -1, 1).astype(I)
    return s * A, s * w0, s * w1, s * w2


def rasterize(meshes, W, H):
    """meshes {meshId: uv (P, 3, 2)} -> (texels (n,) uint32 ascending, hits (n,) HIT_DTYPE, counts dict n / rejected / degenerate /
    pairs)."""
    owner = np.full(W * H, NO_OWNER, dtype=U)
    counts = dict(n=0, rejected=0, degenerate=0, pairs=0)
    snapped = {}
    for m in sorted(meshes):
        X, Y, ok = snap(meshes[m], W, H)
        snapped[m] = (X, Y)
        assert m < 8 and len(X) <= 1 << 28
        for prim in range(len(X)):
            if not ok[prim]:
                counts["rejected"] += 1
                continue
            x, y = X[prim], Y[prim]
            if edge(x[0], y[0], x[1], y[1], x[2], y[2]) == 0:
                counts["degenerate"] += 1
                continue
            # the texels whose centre 256 x + 128 lies in the triangle's box, clipped to the atlas (// floors)
            x0, x1 = max(0, -((128 - int(x.min())) // 256)), min(W - 1, (int(x.max()) - 128) // 256)
            y0, y1 = max(0, -((128 - int(y.min())) // 256)), min(H - 1, (int(y.max()) - 128) // 256)
            if x0 > x1 or y0 > y1:
                continue
            tx, ty = np.meshgrid(np.arange(x0, x1 + 1, dtype=I), np.arange(y0, y1 + 1, dtype=I))
            _, w0, w1, w2 = weights(x, y, 256 * tx + 128, 256 * ty + 128)
            inside = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
            counts["pairs"] += int(inside.sum())
            t = (ty[inside] * W + tx[inside]).astype(I)
            owner[t] = np.minimum(owner[t], U((m << 28) | prim))
    texels = np.nonzero(owner != NO_OWNER)[0].astype(U)
    counts["n"] = len(texels)
    hits = np.zeros(len(texels), dtype=HIT_DTYPE)
    key = owner[texels]
    hits["meshId"], hits["primId"] = key >> 28, key & U((1 << 28) - 1)
    for m in sorted(meshes):
        sel = np.nonzero(hits["meshId"] == m)[0]
        if not len(sel):
            continue
        X, Y = snapped[m][0][hits["primId"][sel]], snapped[m][1][hits["primId"][sel]]
        tx, ty = (texels[sel] % W).astype(I), (texels[sel] // W).astype(I)
        A, w0, w1, w2 = weights(X, Y, 256 * tx + 128, 256 * ty + 128)
        assert (w0 + w1 + w2 == A).all() and (A > 0).all()
        a = A.astype(F)  # int64 to float32: to nearest even
        hits["i"][sel], hits["j"][sel], hits["k"][sel] = w0.astype(F) / a, w1.astype(F) / a, w2.astype(F) / a
    return texels, hits, counts


def points(texels, hits, W, meshes, normals, bias, set_tile):
    """(n,) POINT_DTYPE.  meshes: per mesh of the scene (indices (P, 3), positions (V, 3) float32); normals (n, 3): N of every VALID
    record (prt_hip_query_surface's normal for the same hit; this restatement does not interpolate normals).  A hit whose meshId or
    primId lies outside the scene gives the all-zero point with set = 0xffffffff."""
    texels, hits = np.asarray(texels, dtype=U), np.asarray(hits, dtype=HIT_DTYPE)
    out = np.zeros(len(hits), dtype=POINT_DTYPE)
    out["set"] = NEVER
    x, y = texels % U(W), texels // U(W)
    for m, (idx, pos) in enumerate(meshes):
        idx, pos = np.asarray(idx, dtype=U).reshape(-1, 3), np.asarray(pos, dtype=F).reshape(-1, 3)
        sel = np.nonzero((hits["meshId"] == m) & (hits["primId"] < len(idx)))[0]
        if not len(sel):
            continue
        p0, p1, p2 = (pos[idx[hits["primId"][sel], c]] for c in range(3))
        i, j, k = (hits[name][sel][:, None] for name in "ijk")
        with np.errstate(all="ignore"):
            P = (i * p0 + j * p1) + k * p2
        assert P.dtype == F
        out["P"][sel], out["bias"][sel], out["N"][sel] = P, F(bias), np.asarray(normals, dtype=F)[sel]
        out["set"][sel] = (x[sel] % U(set_tile)) + U(set_tile) * (y[sel] % U(set_tile))
    return out


def resolve(texels, values, W, H, gutter):
    """(image (H * W, stride) float32, mask (H * W,) uint8) of values (n, stride) at texels (n,)."""
    texels = np.asarray(texels, dtype=U).reshape(-1)
    values = np.ascontiguousarray(values, dtype=F).reshape(len(texels), -1)
    stride = values.shape[1]
    image, mask = np.zeros((H, W, stride), dtype=F), np.zeros((H, W), dtype=np.uint8)
    keep = texels < W * H
    assert len(np.unique(texels[keep])) == keep.sum(), "with duplicate indices the stored value is unspecified"
    image.reshape(-1, stride)[texels[keep]] = values[keep]
    mask.reshape(-1)[texels[keep]] = 1
    for g in range(1, gutter + 1):
        src = np.zeros((H + 2, W + 2), dtype=bool)
        src[1:-1, 1:-1] = (mask >= 1) & (mask <= g)
        img = np.zeros((H + 2, W + 2, stride), dtype=F)
        img[1:-1, 1:-1] = image
        s, count = np.zeros((H, W, stride), dtype=F), np.zeros((H, W), dtype=np.int64)
        with np.errstate(all="ignore"):
            for dy in (0, 1, 2):  # dy = -1, 0, 1 outer, dx = -1, 0, 1 inner
                for dx in (0, 1, 2):
                    nb = src[dy:dy + H, dx:dx + W]
                    s = np.where(nb[:, :, None], s + img[dy:dy + H, dx:dx + W], s)
                    count += nb
            fill = (mask == 0) & (count > 0)
            image[fill] = s[fill] / count[fill].astype(F)[:, None]
        mask[fill] = g + 1
        assert image.dtype == F
    return image.reshape(-1, stride), mask.reshape(-1)
