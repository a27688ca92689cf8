"""The definition of include/prt_hip.h "lens renders" restated in numpy: draws(), rays(lens, y0, y1) and accumulate(lens, L, image, y0,
y1), float32 throughout, every product rounded before the sum that uses it, sums left to right as the header writes them, vectorised
over the rays of a band.  sinf and cosf come through ctypes from the machine's libm.so.6 (not np.sin, whose float32 loop need not be
libm's), sqrtf and the divisions are plain float32 operations.  tests/test_lens_cpu.py pins this file against a host program compiled
from prt_amd/csrc/prt_lens.h and against its own properties; tests/test_gpu_lens.py holds the product to it byte for byte (with
prt_bake_ref.same_bytes: a NaN of the restatement asks for a NaN).  Nothing here is product code.

A lens is anything with the fields of prt_lens_desc (prt_amd.LensDesc: `pass` is pass_ there)."""
import ctypes as C

import numpy as np

from prt_bake_ref import RAY_DTYPE, normalize3

F = np.float32
U = np.uint32
PINHOLE, ORTHO, EQUIRECT, FISHEYE = 0, 1, 2, 3
CENTRE, ACCUMULATE = 1, 2
MAX_RAYS = 1 << 24
_libm = C.CDLL("libm.so.6")
for _f in (_libm.sinf, _libm.cosf):
    _f.restype = C.c_float
    _f.argtypes = [C.c_float]


def sincosf(x):
    """(sinf(x), cosf(x)) of libm on every element of a float32 array (each distinct value once)."""
    x = np.asarray(x, dtype=F)
    u, inv = np.unique(x.view(U).reshape(-1), return_inverse=True)
    s = np.array([_libm.sinf(float(v)) for v in u.view(F)], dtype=F)
    c = np.array([_libm.cosf(float(v)) for v in u.view(F)], dtype=F)
    return s[inv].reshape(x.shape), c[inv].reshape(x.shape)


def mix(v):
    """The five steps of pixel_seed without its final | 1, on uint32 arrays (wrapping)."""
    v = np.asarray(v, dtype=U).copy()
    with np.errstate(over="ignore"):
        v ^= v >> U(16)
        v *= U(0x7feb352d)
        v ^= v >> U(15)
        v *= U(0x846ca68b)
        v ^= v >> U(16)
    return v


def xorshift32(s):
    s = s ^ (s << U(13))
    s = s ^ (s >> U(17))
    return s ^ (s << U(5))


def rng_to_float(s):
    return ((s & U(0x007fffff)) | U(0x3f800000)).view(F) - F(1.0)


def draws(lens, x, y, k):
    """(4, n) float32: u0 .. u3 of ray k of pixel (x, y) (uint32 arrays of one length)."""
    x, y, k = (np.asarray(v, dtype=U) for v in (x, y, k))
    with np.errstate(over="ignore"):
        pix = y * U(lens.width) + x
        j = U(lens.pass_ & 0xffffffff) * U(lens.K) + k
        s = mix(mix(pix + U(lens.jitterSeed)) + j) | U(1)
    u = np.zeros((4, len(x)), dtype=F)
    for i in range(4):
        s = xorshift32(s)
        u[i] = rng_to_float(s)
    return u


def _v(a):
    return np.array(list(a), dtype=F)


def band_index(lens, y0, y1):
    """(x, y, k) uint32 of ray r = ((y - y0)*W + x)*K + k, r = 0 .. (y1 - y0)*W*K - 1."""
    yy, xx, kk = np.meshgrid(np.arange(y0, y1, dtype=U), np.arange(lens.width, dtype=U), np.arange(lens.K, dtype=U), indexing="ij")
    return xx.reshape(-1), yy.reshape(-1), kk.reshape(-1)


def film(lens, x, y, u):
    """(a, b) of the header's Film step."""
    centre = bool(lens.flags & CENTRE)
    jx = F(0.5) if centre else u[0]
    jy = F(0.5) if centre else u[1]
    invW, invH = F(1.0) / F(lens.width), F(1.0) / F(lens.height)
    sx = (x.astype(F) + jx) * invW
    sy = (y.astype(F) + jy) * invH
    return F(2.0) * sx - F(1.0), F(1.0) - F(2.0) * sy


def rays(lens, y0=0, y1=None):
    """((y1 - y0) * W * K,) RAY_DTYPE: the rays of rows [y0, y1)."""
    y1 = lens.height if y1 is None else y1
    x, y, k = band_index(lens, y0, y1)
    n = len(x)
    u = draws(lens, x, y, k)
    a, b = film(lens, x, y, u)
    assert a.dtype == F and b.dtype == F
    pos, fwd, right, up = _v(lens.pos), _v(lens.fwd), _v(lens.right), _v(lens.up)
    a1, b1 = a[:, None], b[:, None]
    org = np.broadcast_to(pos, (n, 3)).copy()
    with np.errstate(all="ignore"):
        if lens.model == PINHOLE:
            d = (fwd + a1 * right) + b1 * up
            if not (F(lens.lensRadius) > F(0.0)):
                dr = d
            else:
                rl = F(lens.lensRadius) * np.sqrt(u[2])
                sn, cs = sincosf(F(6.28318530717958647692) * u[3])
                R, Uv = normalize3(right), normalize3(up)
                org = (pos + (rl * cs)[:, None] * R) + (rl * sn)[:, None] * Uv
                Fp = pos + F(lens.focus) * d
                dr = Fp - org
        elif lens.model == ORTHO:
            org = (pos + a1 * right) + b1 * up
            dr = np.broadcast_to(fwd, (n, 3)).copy()
        elif lens.model == EQUIRECT:
            sp, cp = sincosf(a * F(3.14159265358979323846))
            st, ct = sincosf(b * F(1.57079632679489661923))
            dr = ((ct * sp)[:, None] * right + st[:, None] * up) + (ct * cp)[:, None] * fwd
        elif lens.model == FISHEYE:
            rr = np.sqrt(a * a + b * b)
            st, ct = sincosf(rr * (F(0.5) * F(lens.fov)))
            q = np.where(rr > F(0.0), st / np.where(rr > F(0.0), rr, F(1.0)), F(0.0)).astype(F)
            dr = ((a * q)[:, None] * right + (b * q)[:, None] * up) + ct[:, None] * fwd
            dr[~(rr <= F(1.0))] = F(0.0)
        else:
            raise ValueError(lens.model)
    assert org.dtype == F and dr.dtype == F and org.shape == dr.shape == (n, 3)
    out = np.zeros(n, dtype=RAY_DTYPE)  # tMax = 0, pad = 0
    out["org"], out["dir"] = org, dr
    return out


def focus_points(lens, y0=0, y1=None):
    """(n, 3) float32: F = pos + focus*d of every ray of a PINHOLE lens."""
    y1 = lens.height if y1 is None else y1
    x, y, k = band_index(lens, y0, y1)
    a, b = film(lens, x, y, draws(lens, x, y, k))
    d = (_v(lens.fwd) + a[:, None] * _v(lens.right)) + b[:, None] * _v(lens.up)
    return _v(lens.pos) + F(lens.focus) * d


def accumulate(lens, L, image=None, y0=0, y1=None):
    """(H, W, 3) float32: per pixel and component S = +0, S = S + L[r0 + k] for k = 0 .. K-1; the band's rows of `image` (None:
    zeros) become image + S under ACCUMULATE and S otherwise; a new array."""
    W, H, K = lens.width, lens.height, lens.K
    y1 = H if y1 is None else y1
    L = np.ascontiguousarray(L, dtype=F).reshape((y1 - y0) * W, K, 3)
    out = np.zeros((H, W, 3), dtype=F) if image is None else np.array(image, dtype=F).reshape(H, W, 3)
    S = np.zeros(((y1 - y0) * W, 3), dtype=F)
    with np.errstate(all="ignore"):
        for k in range(K):
            S = S + L[:, k]
        S = S.reshape(y1 - y0, W, 3)
        out[y0:y1] = out[y0:y1] + S if lens.flags & ACCUMULATE else S
    assert out.dtype == F
    return out


def band_seed(lens, seed, y0):
    """The seed prt_hip_query_radiance gets for the band that starts at row y0: seed + pass*(W*H*K) + y0*W*K, uint32 wrap."""
    W, H, K = lens.width, lens.height, lens.K
    return (seed + lens.pass_ * ((W * H * K) & 0xffffffff) + y0 * W * K) & 0xffffffff


def bands(lens):
    """[(y0, y1)] of prt_hip_lens_render: ascending, as many rows as fit 2^24 probes, or bandRows if that is fewer."""
    rows = min(lens.height, MAX_RAYS // (lens.width * lens.K))
    rows = min(rows, lens.bandRows) if lens.bandRows else rows
    return [(y, min(lens.height, y + rows)) for y in range(0, lens.height, rows)]
