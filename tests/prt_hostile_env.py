"""Hostile environment maps and draws for InfiniteAreaLight::sample (light.cpp:86-128; env_sample / cdf_find in prt_device.h, env_sample
in prt_oracle.c): tests/test_hostile_env_cpu.py, tests/test_gpu_hostile_env.py.

Everything is deterministic (np.random.default_rng(SEED)); tests/golden/make_golden.py stores the inputs with the answers of the COMPILED
reference (oracle/_ref/ref_path envlight / render) in tests/golden/hostile_env.npz, so that the tests do not depend on numpy's generator
staying what it is.

Maps    maps(): float RGBA (h, w, 4), one line of why beside each.  refused_maps() are the ones every way into the library refuses.
Draws   per map (draws()): Y = 0, 1 - 2^-23, 0.5 and, for every finite entry v of the vertical table, v, its two float neighbours, v floored
        to the generator's grid k * 2^-23 and the grid point above that; for every u.y the row the reference's scan selects, and X built
        the same way from that row's entries (all of them up to PICK, a seeded pick that holds entry 0, the last one and the two around
        `first` beyond) plus 0, 0.5 and 1 - 2^-23.  Y is thinned by a seeded choice -- never its two ends nor the values around `first`
        -- until all maps together give at most MAX_DRAWS draws.
undefined   a draw whose u.y no vertical entry exceeds (after one that differs from its predecessor): the reference leaves y == height
        and reads one row past its horizontal table.  The kernel and the oracle define it (xf = 0, pdfH = 1); the reference's answers
        there are stored as zeros and never compared."""
import os

import numpy as np

import prt_testlib as T

F = np.float32
SEED = 20261021
GRID = F(2.0 ** -23)
TOP = F(1.0) - GRID          # the generator's largest draw (random.h: mantissa bits | 1.0f, minus 1)
MAX_DRAWS = 16000
PICK = 24
GOLDEN_FILE = os.path.join(T.GOLDEN, "hostile_env.npz")
RENDER = (40, 40, 8)         # width, height, samples of the whole-frame cases


# ----------------------------------------------------------------------------- maps
def _rgba(rgb):
    e = np.ones(rgb.shape[:2] + (4,), dtype=F)
    e[..., :3] = rgb
    return e


def maps():
    """[(name, env (h, w, 4) float32)], every one accepted by the library."""
    rng = np.random.default_rng(SEED)
    noise = lambda w, h: rng.uniform(0.05, 2.0, (h, w, 3)).astype(F)  # noqa: E731
    # the smallest map with a search in both directions; a horizontal table of one entry (the search always returns the width); a
    # vertical table of one entry (always y == height: every draw is undefined in the reference)
    out = [("2x2", _rgba(noise(2, 2))), ("w1", _rgba(noise(1, 8))), ("h1", _rgba(noise(8, 1)))]
    e = np.zeros((6, 9, 3), dtype=F)   # one lit texel in column 0: rows 0-2, 4, 5 are NaN rows, row 3 is 1, 1, ..., 1 (`first` = width)
    e[3, 0] = (2.0, 3.0, 4.0)
    out.append(("one_texel", _rgba(e)))
    e = T.sky_env(24, 12)[..., :3]     # entry 0 of the vertical table exceeds nearly half of all draws (the map of tests/test_gpu_parity.py)
    e[0, 0] = 5000.0
    out.append(("bright_first", _rgba(e)))
    e = T.sky_env(24, 12, seed=9)[..., :3]  # plateaus at both ends of both tables, NaN rows first and last
    e[0], e[-1], e[:, 0], e[:, -1] = 0.0, 0.0, 0.0, 0.0
    out.append(("black_border", _rgba(e)))
    e = noise(16, 8)
    e[:, 1::2] = 0.0                   # rows a, a, b, b, ...: `first` = 2 with cdf[0] > u for small u
    out.append(("plateaus", _rgba(e)))
    # 40 decades of radiance: increments that vanish in the running sums, rows that cross PRT_ENV_CHUNK, a table that ends above 1.
    # Row 4 begins with two tiny texels, t0 = 54.5 * t1: u.x = 0 selects entry 1 with pdfH = t1 / (the row's sum) ~ 1e-32 and the offset
    # -t0 / t1, which wraps onto the centre of column 10, lit with 1e10 in rows 3 and 4 -- the colour overflows to inf.
    e = (10.0 ** rng.uniform(-30.0, 10.0, (8, 65, 1))).astype(F) * np.ones(3, dtype=F)
    e[4, 0], e[4, 1], e[3:5, 10] = F(54.5e-22), F(1e-22), F(1e10)
    out.append(("range", _rgba(e)))
    out.append(("flat", _rgba(np.ones((4, 300, 3), dtype=F))))   # a long table: the rounding drift of 300 equal steps
    out.append(("negative", _rgba(-noise(16, 16))))              # the length is positive, the colour negative: the map is accepted
    e = noise(12, 6)                   # row 1 and column 1 black under a bright row 0 / column 0: `first` = 2 in both tables
    e[0] *= F(8.0)
    e[:, 0] *= F(8.0)
    e[1], e[:, 1] = 0.0, 0.0
    out.append(("second_black", _rgba(e)))
    # Row 0 and column 0 outshine the rest: entry 0 of the vertical table and of every row exceeds nearly every draw and the next steps
    # are small, so the offsets (u - prev) / pdf are large and negative and |theta|, |phi| go from 0 into the thousands.  (The scan never
    # returns index 0, so the horizontal row of texel row 0 is never used: bright_first's one texel alone does not take theta that far.)
    e = noise(12, 6)
    e[0] *= F(1e6)
    e[1:, 0] *= F(3000.0)
    out.append(("bright_edge", _rgba(e)))
    return out


def refused_maps():
    """[(name, env, flags of prt_amd.env_tables_host)]: 1 = the vertical table is not non-decreasing, 4 = a row is not.
    subnormal: every length underflows to 0, so this is the black map; black: vsum = 0, the vertical table is 0 * inf = NaN throughout;
    +inf: that row's sum is inf, its table 0, ..., 0, then 0 * inf = NaN from the texel on (4), and the vertical table NaN from that row
    on (1); NaN: that row's table is NaN throughout (allowed, it is what a black row gives) but vsum, hence the vertical table, is NaN."""
    sky = T.sky_env(16, 8)
    sub, black, inf, nan = sky.copy(), sky.copy(), sky.copy(), sky.copy()
    sub[..., :3] = F(1e-42)
    black[..., :3] = 0.0
    inf[3, 5, 0] = np.inf
    nan[3, 5, 1] = np.nan
    return [("subnormal", sub, 1), ("black", black, 1), ("inf", inf, 1 | 4), ("nan", nan, 1)]


REFUSAL_MESSAGE = "vertical CDF is not non-decreasing"  # env_refusal (prt_edit.hip) and prt_hip_upload_scene report flag 1 first


# ----------------------------------------------------------------------------- the two searches
def scan(cdf, u):
    """The reference's linear scan (light.cpp:93-104, :108-119) for every u: the first index i >= 1 with cdf[i] > u whose difference
    to cdf[i - 1] is not 0; len(cdf) when there is none."""
    cdf, u = np.asarray(cdf, dtype=F), np.atleast_1d(np.asarray(u, dtype=F))
    n = len(cdf)
    if n < 2:
        return np.full(len(u), n, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        step = ~((cdf[1:] - cdf[:-1]) == 0)
        ok = (cdf[None, 1:] > u[:, None]) & step[None, :]
    return np.where(ok.any(axis=1), ok.argmax(axis=1) + 1, n)


def first_step(cdf):
    """First index i >= 1 whose value differs from its predecessor's; len(cdf) when there is none (prt_env_first_step)."""
    cdf = np.asarray(cdf, dtype=F)
    with np.errstate(invalid="ignore"):
        step = np.nonzero(~((cdf[1:] - cdf[:-1]) == 0))[0]
    return int(step[0]) + 1 if len(step) else len(cdf)


def cdf_find(cdf, first, u):
    """cdf_find of prt_device.h, statement for statement, for every u: bisection for the upper bound in [1, n), then the `first`
    constant when already cdf[0] > u."""
    cdf, u = np.asarray(cdf, dtype=F), np.atleast_1d(np.asarray(u, dtype=F))
    n = len(cdf)
    lo, hi = np.full(len(u), 1, dtype=np.int64), np.full(len(u), n, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        while True:
            live = lo < hi
            if not live.any():
                break
            mid = (lo + hi) >> 1
            above = cdf[np.minimum(mid, n - 1)] > u
            hi = np.where(live & above, mid, hi)
            lo = np.where(live & ~above, mid + 1, lo)
        patch = (lo == 1) & (lo < n) & (cdf[0] > u)
    return np.where(patch, first, lo)


# ----------------------------------------------------------------------------- draws
def tables(env):
    """(vertical (h,), horizontal (h, w)) of `env` from the oracle, which tests/test_hostile_env_cpu.py pins to the compiled reference's."""
    h, w, _ = env.shape
    o = T.OracleScene(T.SceneDesc([], (0, 0, 1), (0, 0, -1), 8, 8, env=env))
    v, hor = o.env_tables()
    o.close()
    return v, hor.reshape(h, w)


def _unique_in_order(values):
    values = np.asarray(values, dtype=F)
    _, idx = np.unique(values.view(np.uint32), return_index=True)
    return values[np.sort(idx)]


def beside(entries):
    """Every finite entry v with its two float neighbours, v floored to the grid and the grid point above; those in [0, 1)."""
    v = np.asarray(entries, dtype=F)
    v = v[np.isfinite(v)]
    floor = (np.floor(v.astype(np.float64) * 2.0 ** 23) / 2.0 ** 23).astype(F)
    c = np.concatenate([v, np.nextafter(v, F(-np.inf)), np.nextafter(v, F(np.inf)), floor, (floor + GRID).astype(F)]).astype(F)
    return c[(c >= 0) & (c < 1)]


def _x_values(row, rng):
    finite = np.nonzero(np.isfinite(row))[0]
    if len(finite) > PICK:
        f = first_step(row)
        must = np.unique([i for i in (0, len(row) - 1, f - 1, f) if i < len(row) and np.isfinite(row[i])])
        rest = np.setdiff1d(finite, must)
        finite = np.sort(np.concatenate([must, rng.choice(rest, PICK - len(must), replace=False)]))
    return _unique_in_order(np.concatenate([np.array([0.0, 0.5, TOP], dtype=F), beside(row[finite])]))


def draws(maps_list=None):
    """{name: (u (N, 2) float32 {u.x, u.y}, undefined (N,) bool)} for every map, thinned to MAX_DRAWS draws in all."""
    maps_list = maps() if maps_list is None else maps_list
    per_map = []
    for m, (name, env) in enumerate(maps_list):
        v, hor = tables(env)
        h, w = hor.shape
        f = first_step(v)
        must = _unique_in_order(np.concatenate([np.array([0.0, TOP, 0.5], dtype=F), beside(v[[i for i in (f - 1, f) if i < h]])]))
        ys = _unique_in_order(np.concatenate([must, beside(v)]))
        optional = ys[len(must):]
        optional = optional[np.random.default_rng([SEED, m, 1000003]).permutation(len(optional))]
        xs = {h: np.array([0.0, 0.5, TOP], dtype=F)}
        for y in range(1, h):
            xs[y] = _x_values(hor[y], np.random.default_rng([SEED, m, y]))
        per_map.append((name, v, must, optional, xs))

    def build(keep):
        out = {}
        for name, v, must, optional, xs in per_map:
            ys = np.concatenate([must, optional[:int(np.ceil(keep * len(optional)))]])
            rows = scan(v, ys)
            u = np.concatenate([np.stack([xs[int(r)], np.full(len(xs[int(r)]), y, dtype=F)], axis=1) for y, r in zip(ys, rows)])
            out[name] = (np.ascontiguousarray(u, dtype=F), np.repeat(rows == len(v), [len(xs[int(r)]) for r in rows]))
        return out

    for keep in np.linspace(1.0, 0.0, 41):
        out = build(keep)
        if sum(len(u) for u, _ in out.values()) <= MAX_DRAWS:
            return out
    raise AssertionError("the mandatory draws alone exceed MAX_DRAWS")


def generate():
    """dict of every input array of the fixture: <name>/texels, <name>/u, <name>/undefined."""
    out = {}
    maps_list = maps()
    d = draws(maps_list)
    for name, env in maps_list:
        out[f"{name}/texels"] = env
        out[f"{name}/u"] = d[name][0]
        out[f"{name}/undefined"] = d[name][1].astype(np.uint8)
    return out


def always_defined(vertical):
    """No draw of the generator runs off this vertical table: a whole render under the map is defined in the reference."""
    return len(vertical) >= 2 and int(scan(vertical, TOP)[0]) < len(vertical)


# ----------------------------------------------------------------------------- the fixture
_golden = None


def golden():
    """The fixture as {name: dict(texels, u, undefined (bool), ref_vertical, ref_horizontal (h, w), ref_dir, ref_color[, ref_image,
    ref_rays])} in the order of maps()."""
    global _golden
    if _golden is None:
        z = np.load(GOLDEN_FILE)
        g = {}
        for key in z.files:  # (the archive keeps the order in which make_golden.py stored the maps)
            name, field = key.split("/")
            g.setdefault(name, {})[field] = z[key]
        for d in g.values():
            d["undefined"] = d["undefined"].astype(bool)
            d["ref_horizontal"] = d["ref_horizontal"].reshape(d["texels"].shape[:2])
        _golden = g
    return _golden


def ref_words(d):
    """(N, 6) uint32 words {dir, color} of the compiled reference's stored answers."""
    return np.ascontiguousarray(np.concatenate([d["ref_dir"], d["ref_color"]], axis=1), dtype=F).view(np.uint32)


def oracle_scene(env):
    return T.OracleScene(T.SceneDesc([], (0, 0, 1), (0, 0, -1), 8, 8, env=env))


def oracle_words(env, u):
    """(N, 6) uint32 words {dir, color} of the live oracle."""
    o = oracle_scene(env)
    d, c = o.env_sample(u)
    o.close()
    return np.concatenate([d, c], axis=1).view(np.uint32)


def render_desc(env):
    """The Cornell box without the teapot at RENDER's size under `env` (the reference harness and the oracle render this)."""
    desc = T.cornell_scene(RENDER[0], RENDER[1], with_teapot=False)
    desc.env = np.ascontiguousarray(env, dtype=F)
    return desc


def theta_phi(v, hor, u):
    """(theta, phi) of light.cpp:121-122 as float64 approximations, from the tables: only to count how far the angles go."""
    h, w = hor.shape
    th, ph = np.zeros(len(u)), np.zeros(len(u))
    rows = scan(v, u[:, 1])
    for i, (ux, uy) in enumerate(u.astype(np.float64)):
        y, xf, yf = int(rows[i]), 0.0, 0.0
        if y < h:
            yf = y + (uy - float(v[y - 1])) / (float(v[y]) - float(v[y - 1])) - 1.0
            x = int(scan(hor[y], F(ux))[0])
            if x < w:
                xf = x + (ux - float(hor[y, x - 1])) / (float(hor[y, x]) - float(hor[y, x - 1])) - 1.0
        th[i], ph[i] = 2.0 * np.pi * (xf / w + 0.5), np.pi * yf / h
    return th, ph
