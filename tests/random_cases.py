"""Pure case generators of the seeded random sweeps (tests/test_gpu_random.py,
tests/test_gpu_random_queries.py, tests/test_gpu_random_transfer.py and the CPU
census tests/test_random_cases.py; at the end of the file PLANE_SWEEPS, the sweeps of
tests/test_gpu_random_shading.py and tests/test_gpu_random_planes.py with the census
tests/test_random_planes.py).

No GPU and no library: numpy only.  Every generator maps a seed to a plain dict of
Python values -- dims, bins or K, dtype, method and query state, W and H, the
camera as (kind, rotation, translation) for camera.display_inv_view, the render
parameters, baked or per step, tuning knobs -- so a case can be printed whole in a
failure message and rebuilt from its seed.

Cameras are the four kinds of test_gpu_random.draw_camera, whose random stream
draw_view reproduces draw for draw:
  0  row-aligned (no rotation), shifted and zoomed,
  1  exact quarter turns about x and y,
  2  the eye inside the volume, any rotation,
  3  any rotation, the eye outside.

Render parameters: the density is log-uniform in [0.005, 0.5] (rays of a few
hundred samples that leave the box unsaturated, and rays that saturate within 6).
The transfer function is transparent at both ends of its window, and most query
statistics pile up at the ends of their range (a range probability is mostly 0
or 1), so a window drawn blindly misses the statistic in one frame of three.  The
window is therefore drawn per statistic: with SPAN[stat] = (a, b) the nominal
range of the statistic, a maps to 0.08-0.25 of the window and b - a covers
0.35-0.85 of it, so both ends of the range are coloured in most frames and b runs
off the window's end in some.  One case in eight keeps a blind window (offset in
[-0.2, 0.2], scale in [0.5, 2]).

The table sweeps (tf_case, tf2_case, tf_tile_case: frames from baked planes under a
user-defined 1-D or 2-D table) draw each axis' window by the same rule
(draw_window); a user table has no transparent ends, so nearly every frame that
hits the volume is nonzero.  What they deal, so that it is guaranteed: the volume's
family, the methods of the axes, the table's shape and the kind of its entries, an
edge shape for one volume in four, a negated window for one case in eight, the
knobs.
"""
import math

import numpy as np

KINDS = ("row-aligned", "quarter turns", "eye inside", "oblique")
KNOBS = ({}, {"VR_WG_PER_CU": "2"}, {"VR_PAD": "3,5"})
QUERY_BINS = (1, 2, 3, 4, 5, 7, 8, 8, 16, 31, 32)
INSTANCE_BINS = (1, 2, 4, 8, 16, 32)   # bin counts f16 records and the queries are compiled for
METRICS = ("l1", "emd", "ks")

# nominal range of each statistic on the synthetic volumes (see the module docstring)
SPAN = {"weights": (-1.0, 2.0), "range": (0.0, 1.0), "quantile": (0.0, 1.0),
        "spread": (0.0, 0.3), "distance": (0.0, 1.0), "crossing": (0.0, 1.0),
        "mean": (0.0, 1.0), "variance": (0.0, 0.5), "entropy": (0.0, 0.7),
        "gmm mean": (0.0, 0.25), "gmm variance": (0.0, 0.15),
        "gmm quantile": (0.0, 1.0), "gmm spread": (0.0, 0.25)}


def draw_view(rng, kind=None):
    """(kind, (rx, ry), (tx, ty, tz)): test_gpu_random.draw_camera's draws, in its
    order.  kind given: that kind's rotation and translation only."""
    if kind is None:
        kind = int(rng.integers(0, 4))
    if kind == 0:
        rot = (0.0, 0.0)
        tr = (rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), -rng.uniform(1.2, 6.0))
    elif kind == 1:
        rot = tuple(float(rng.choice([0, 90, 180, 270])) for _ in range(2))
        tr = (0.0, 0.0, -rng.uniform(2.5, 5.0))
    elif kind == 2:
        rot = (rng.uniform(-180, 180), rng.uniform(-180, 180))
        tr = (rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5))
    else:
        rot = (rng.uniform(-180, 180), rng.uniform(-180, 180))
        tr = (rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), -rng.uniform(1.5, 6.0))
    return kind, tuple(float(v) for v in rot), tuple(float(v) for v in tr)


def _f32(x):
    return float(np.float32(x))


def draw_window(rng, stat):
    """(offset, scale) of a transfer window for the statistic `stat`: the module
    docstring's rule, one in eight blind"""
    blind = bool(rng.integers(0, 8) == 0)
    u, v = rng.uniform(), rng.uniform()
    if blind:
        toff, tscale = -0.2 + 0.4 * u, 0.5 + 1.5 * v
    else:
        a, b = SPAN[stat]
        tscale = (0.35 + 0.5 * v) / (b - a)
        toff = a - (0.08 + 0.17 * u) / tscale
    return _f32(toff), _f32(tscale)


def draw_params(rng, stat):
    """density, brightness and the transfer window for the statistic `stat`"""
    density = _f32(math.exp(rng.uniform(math.log(0.005), math.log(0.5))))
    brightness = _f32(rng.uniform(0.5, 2.0))
    toff, tscale = draw_window(rng, stat)
    return dict(density=density, brightness=brightness, toff=toff, tscale=tscale)


def _knobs(rng):
    return dict(KNOBS[int(rng.integers(0, len(KNOBS)))])


def _ordered_pair(rng, lo=0.0, hi=1.0):
    a, b = sorted(_f32(v) for v in rng.uniform(lo, hi, 2))
    if a == b:
        b = _f32(min(hi, a + 0.125))
    return a, b


def draw_query(rng, method, nb, dims, deal=None):
    """(query state, the statistic's name in SPAN) of a histogram query; deal: a
    counter that deals method 12's metric and similarity flag instead of the draw"""
    if method == 10:
        if rng.integers(0, 2):
            return {"state": "weights", "wseed": int(rng.integers(1, 1 << 20))}, "weights"
        lo, hi = _ordered_pair(rng)
        return {"state": "range", "lo": lo, "hi": hi}, "range"
    if method == 11:
        k = int(rng.integers(0, 4))
        if k == 0:
            return {"state": "q", "q": float(rng.integers(0, 2))}, "quantile"
        if k == 1:
            lo, hi = _ordered_pair(rng)
            return {"state": "spread", "lo": lo, "hi": hi}, "spread"
        return {"state": "q", "q": _f32(rng.uniform(0.02, 0.98))}, "quantile"
    if method == 12:
        q = {"metric": METRICS[int(rng.integers(0, 3))], "similarity": bool(rng.integers(0, 2))}
        if deal is not None:  # the 3 x 2 combinations in turn
            q = {"metric": METRICS[deal % 3], "similarity": bool((deal // 6) % 2)}
        if rng.integers(0, 2):
            h = rng.random(nb) + 0.05
            q.update(state="target", target=[_f32(v) for v in h / h.sum()])
        else:  # a box of at most 8 x 8 x 8 voxels
            lo, hi = [], []
            for n in dims:
                a = int(rng.integers(0, n))
                lo.append(a)
                hi.append(int(rng.integers(a + 1, min(n, a + 8) + 1)))
            q.update(state="region", lo=tuple(lo), hi=tuple(hi))
        return q, "distance"
    assert method == 13
    return {"state": "isovalue", "theta": _f32(rng.uniform(0.05, 0.95))}, "crossing"


def _frame(rng, wmax, hmax):
    return int(rng.integers(1, wmax + 1)), int(rng.integers(1, hmax + 1))


def hist_query_case(seed):
    """a whole frame of query method 10 / 11 / 12 / 13 on a histogram volume.
    Only fp32 records draw the bin counts the queries have no instance for (3, 5,
    7, 31: the library refuses the query, `supported` False).  Method, dtype,
    baked / per step (one in three baked) and the bin count are dealt by the seed,
    so that every method meets every bin count in both dtypes; the rest is random."""
    rng = np.random.default_rng(7000 + seed)
    method = (10, 11, 12, 13)[seed % 4]
    dtype = ("f32", "f16")[(seed // 4) % 2]
    turn = seed // 8            # 0 .. 11 within a method and dtype
    baked = turn % 3 == 0
    dims = tuple(int(v) for v in rng.integers(2, 33, 3))
    bins = QUERY_BINS if dtype == "f32" else tuple(b for b in QUERY_BINS if b in INSTANCE_BINS)
    nb = int(bins[(turn + 3 * (seed % 4)) % len(bins)])
    W, H = _frame(rng, 96, 72)
    kind, rot, tr = draw_view(rng)
    query, stat = draw_query(rng, method, nb, dims, deal=seed // 4)
    return dict(sweep="hist", seed=seed, dims=dims, nb=nb, dtype=dtype, method=method, query=query,
                stat=stat, W=W, H=H, kind=kind, rotation=rot, translation=tr,
                params=draw_params(rng, stat), baked=baked, knobs=_knobs(rng),
                supported=nb in INSTANCE_BINS)


def hist_tile_case(seed):
    """a frame of a query method split over 2-8 ranks' tile lists"""
    rng = np.random.default_rng(7500 + seed)
    dims = tuple(int(v) for v in rng.integers(2, 33, 3))
    dtype = ("f32", "f16")[int(rng.integers(0, 2))]
    nb = int(rng.choice([1, 2, 4, 8, 8, 16, 32]))
    method = int(rng.choice([10, 11, 12, 13]))
    W, H = _frame(rng, 200, 120)
    world = 2 + seed % 7   # dealt: every world size 2-8 occurs
    kind, rot, tr = draw_view(rng)
    query, stat = draw_query(rng, method, nb, dims)
    return dict(sweep="tiles", seed=seed, dims=dims, nb=nb, dtype=dtype, method=method,
                query=query, stat=stat, W=W, H=H, world=world, kind=kind, rotation=rot,
                translation=tr, params=draw_params(rng, stat),
                baked=bool(rng.integers(0, 3) == 0), knobs=_knobs(rng), supported=True)


def f16_case(seed):
    """methods 1 / 2 / 3 / 7 of an f16 record volume, per step or from bake_stats.
    An f16 volume has no per-step march of method 7 (it reads the baked corner
    means), so a method-7 case is always baked; its grid is the volume's or another.
    Method and bin count are dealt by the seed: every pair occurs twice, the first
    time per step, the second time per step or baked in turn."""
    rng = np.random.default_rng(8000 + seed)
    dims = tuple(int(v) for v in rng.integers(2, 33, 3))
    method = (1, 2, 3, 7)[seed % 4]
    nb = INSTANCE_BINS[(seed // 4) % 6]
    W, H = _frame(rng, 96, 72)
    kind, rot, tr = draw_view(rng)
    baked = (seed >= 24 and (seed // 4 + seed) % 2 == 0) or method == 7
    m7 = tuple(int(v) for v in rng.integers(2, 33, 3)) if rng.integers(0, 2) else dims
    stat = {1: "mean", 2: "variance", 3: "entropy", 7: "mean"}[method]
    return dict(sweep="f16", seed=seed, dims=dims, nb=nb, dtype="f16", method=method, W=W, H=H,
                kind=kind, rotation=rot, translation=tr, params=draw_params(rng, stat),
                baked=baked, m7=m7, knobs=_knobs(rng))


def draw_gmm_query(rng, dtype, deal, chain=False):
    """(what, method, query state, statistic).  Mean and variance on f16 records only
    (test_gpu_random sweeps the fp32 march) except in chains; the crossing of the
    range plane (method 13) only in whole-volume cases, where it is always baked.
    The counter `deal` deals the statistic, and with it the spread (one quantile
    case in three) and the infinite bounds (two range cases in six); the values are
    random."""
    whats = ["range", "quantile"] + (["mean", "variance"] if dtype == "f16" or chain else []) \
        + ([] if chain else ["crossing"])
    what, turn = whats[deal % len(whats)], deal // len(whats)
    if what in ("mean", "variance"):
        return what, 1 if what == "mean" else 2, {}, "gmm " + what
    if what == "range":
        lo, hi = _ordered_pair(rng)
        if turn % 6 == 0:
            lo = -math.inf
        elif turn % 6 == 1:
            hi = math.inf
        return what, 10, {"lo": lo, "hi": hi}, "range"
    if what == "quantile":
        if turn % 3 == 0:
            lo, hi = _ordered_pair(rng)
            return what, 11, {"state": "spread", "lo": lo, "hi": hi}, "gmm spread"
        return what, 11, {"state": "q", "q": _f32(rng.uniform(0.02, 0.98))}, "gmm quantile"
    return what, 13, {"theta": _f32(rng.uniform(0.1, 0.9))}, "crossing"


def gmm_case(seed):
    """a whole frame of a GMM volume: mean / variance (f16), the range probability,
    the quantile or the crossing of the range plane; per step or from its plane.
    The dtype alternates with the seed and the statistic is dealt (draw_gmm_query);
    per step and baked alternate with each round of the statistics."""
    rng = np.random.default_rng(8500 + seed)
    dims = tuple(int(v) for v in rng.integers(2, 25, 3))
    K = int(rng.choice([8, 16, 32]))
    dtype = ("f32", "f16")[seed % 2]
    what, method, query, stat = draw_gmm_query(rng, dtype, seed // 2)
    W, H = _frame(rng, 96, 72)
    kind, rot, tr = draw_view(rng)
    baked = bool((seed // 2 // (5 if dtype == "f16" else 3)) % 2) or what == "crossing"
    return dict(sweep="gmm", seed=seed, dims=dims, K=K, dtype=dtype, what=what, method=method,
                query=query, stat=stat, W=W, H=H, kind=kind, rotation=rot, translation=tr,
                params=draw_params(rng, stat), baked=baked, knobs=_knobs(rng))


CHAIN_REDRAWS = 8


def gmm_chain_case(seed, direction):
    """a chain of 2-4 z-slabs of a GMM volume, method 1 / 2 or the range or quantile
    query.  direction(rotation, translation, W, H) is slabs.march_direction of that
    camera: while it is 0 (rays cross z both ways: no chain) the camera is drawn
    again, at most CHAIN_REDRAWS times within its kind (one case in three is of the
    eye-inside kind, the others draw theirs), then the rotation is dropped (every
    ray steps towards -z).  Slab count, dtype and statistic are dealt by the seed."""
    rng = np.random.default_rng(9000 + seed)
    nslabs = 2 + (seed // 2) % 3
    dims = tuple(int(v) for v in rng.integers(4, 25, 3))
    K = int(rng.choice([8, 16, 32]))
    dtype = ("f32", "f16")[(seed // 4) % 2]
    what, method, query, stat = draw_gmm_query(rng, dtype, seed, chain=True)
    W, H = _frame(rng, 96, 72)
    kind = 2 if rng.integers(0, 3) == 0 else int(rng.integers(0, 4))
    _, rot, tr = draw_view(rng, kind)
    redraws = 0
    while direction(rot, tr, W, H) == 0 and redraws < CHAIN_REDRAWS:
        _, rot, tr = draw_view(rng, kind)
        redraws += 1
    if direction(rot, tr, W, H) == 0:
        rot = (0.0, 0.0)
    return dict(sweep="chain", seed=seed, nslabs=nslabs, dims=dims, K=K, dtype=dtype, what=what,
                method=method, query=query, stat=stat, W=W, H=H, kind=kind, rotation=rot,
                translation=tr, redraws=redraws, params=draw_params(rng, stat), knobs=_knobs(rng))


# ---- frames from baked planes under a user-defined table (tests/test_gpu_random_transfer.py) ----

# twelve seeds deal 7 record, 2 codec and 3 GMM volumes
FAMILIES = ("records", "codec", "records", "gmm", "records", "records", "codec", "records",
            "gmm", "records", "gmm", "records")
TF_METHODS = {"records": (1, 2, 3, 10, 11, 12, 13), "codec": (4, 5, 6), "gmm": (1, 2, 10, 11, 13)}
EDGE_NX = (2, 15, 16, 17, 31, 32)   # around the 15-voxel pitch of the planes' 16-wide bricks
EDGE_NY = (2, 3, 5)                 # one brick of two rows, and odd row counts
TF_SIZES = (1, 2, 3, 9, 17, 255, 256)
# (nv, nu): one entry, one row, one column, 1024 entries both ways (many rows: nv = 256),
# the square, the smallest with both axes, odd sides, and 1020 entries (three whole
# staging rounds of 256 threads and a partial fourth)
TF2_SHAPES = ((1, 1), (1, 256), (256, 1), (4, 256), (256, 4), (32, 32), (2, 2), (3, 7), (5, 204))
TABLE_KINDS = ("unit", "8bit", "wide")
TF_KNOBS = KNOBS + ({"VR_TF_WIDE": "1"},)
_RAW_STATS = {1: "mean", 2: "variance", 3: "entropy", 4: "mean", 5: "variance", 6: "entropy"}


def _turn(seed):
    """(family, how many smaller seeds have that family)"""
    family = FAMILIES[seed % 12]
    return family, sum(FAMILIES[s % 12] == family for s in range(seed))


def make_table(table):
    """the float32 table of a case's `table` entry: (n, 4) or (nv, nu, 4).  unit:
    uniform in [0, 1); 8bit: k / 255; wide: RGB in [-0.5, 2), alpha in [-0.25, 1.5)
    (an alpha outside [0, 1] is legal: nothing in the table is clamped)"""
    rng = np.random.default_rng(table["seed"])
    shape = tuple(table["shape"]) + (4,)
    if table["kind"] == "unit":
        t = rng.random(shape)
    elif table["kind"] == "8bit":
        t = rng.integers(0, 256, shape).astype(np.float32) / np.float32(255)
    else:
        t = rng.uniform(-0.5, 2.0, shape)
        t[..., 3] = rng.uniform(-0.25, 1.5, shape[:-1])
    t = np.ascontiguousarray(t, dtype=np.float32)
    assert np.isfinite(t).all()
    return t


def _gmm_axis_query(rng, dtype, method, turn):
    """draw_gmm_query's state of GMM method 10, 11 or 13: its range, quantile or theta"""
    whats = ["range", "quantile"] + (["mean", "variance"] if dtype == "f16" else []) + ["crossing"]
    what = {10: "range", 11: "quantile", 13: "crossing"}[method]
    _, got, query, stat = draw_gmm_query(rng, dtype, whats.index(what) + len(whats) * turn)
    assert got == method
    return query, stat


def draw_axis_queries(rng, family, methods, nb, dims, dtype, turn):
    """draw_query (draw_gmm_query for a GMM volume) once per distinct method of a
    frame's axes: ({method: query state}, {method: the statistic's name in SPAN}).
    A record pair (10, 13) holds both the range or weights and the isovalue.  On a
    GMM volume 10 and 13 read one plane, the range plane: with both in a frame the
    range is 13's (-inf, theta)."""
    queries, stats = {}, {}
    for m in dict.fromkeys(methods):
        if m <= 6:
            stats[m] = ("gmm " if family == "gmm" else "") + _RAW_STATS[m]
        elif family == "records":
            queries[m], stats[m] = draw_query(rng, m, nb, dims)
        elif m == 10 and 13 in methods:
            continue
        else:
            queries[m], stats[m] = _gmm_axis_query(rng, dtype, m, turn)
    if family == "gmm" and 10 in methods and 13 in methods:
        queries[10] = {"lo": -math.inf, "hi": queries[13]["theta"]}
        stats[10] = "range"
    return queries, stats


def _negated(stat, off, scale):
    """the window mirrored: the scale negated and the offset moved to the other end
    of the statistic's span, so SPAN's ends exchange their places in the table"""
    a, b = SPAN[stat]
    return _f32(a + b - off), _f32(-scale)


def _tf_volume(rng, seed, family, turn, methods):
    """what a table case shares with its volume: dims (one seed in four is dealt an
    edge nx and ny), bins or K, dtype, the query state of the methods"""
    lo_hi = (2, 25) if family == "gmm" else (2, 33)
    dims = tuple(int(v) for v in rng.integers(*lo_hi, 3))
    edge = (seed + seed // 12) % 4 == 1
    if edge:
        dims = (EDGE_NX[(seed // 4) % 6], EDGE_NY[(seed // 4 + seed // 24) % 3], dims[2])
    dtype = ("f32", "f16")[turn % 2]
    c = dict(family=family, dims=dims, edge=edge, dtype=dtype)
    if family == "gmm":
        c["K"] = (8, 16, 32)[turn % 3]
        nb = None
    else:
        nb = c["nb"] = INSTANCE_BINS[(turn // 2) % 6]
        if family == "codec":  # (one dtype: every bin count in six turns)
            c["dtype"], nb = "f32", INSTANCE_BINS[turn % 6]
            c["nb"] = nb
    c["queries"], c["stats"] = draw_axis_queries(rng, family, methods, nb, dims, dtype, turn)
    return c


def _tf_rest(rng, seed, c, u, v, wmax, hmax):
    """frame, view, windows, table and knobs of a table case; v None: a 1-D table"""
    c["W"], c["H"] = _frame(rng, wmax, hmax)
    tiny = seed % 24 == 7   # dealt: a 1 x 1 frame, seen from inside so that its ray hits
    if tiny:
        c["W"], c["H"] = 1, 1
    c["kind"], c["rotation"], c["translation"] = draw_view(rng, 2 if tiny else None)
    c["params"] = draw_params(rng, c["stats"][u])
    negate = seed % 8 == 5
    flip_v = negate and v is not None and (seed // 8) % 2 == 1
    if v is not None:
        c["voff"], c["vscale"] = draw_window(rng, c["stats"][v])
        if flip_v:
            c["voff"], c["vscale"] = _negated(c["stats"][v], c["voff"], c["vscale"])
        shape = TF2_SHAPES[(seed + seed // 9) % 9]
    else:
        shape = (TF_SIZES[seed % 7],)
    if negate and not flip_v:
        p = c["params"]
        p["toff"], p["tscale"] = _negated(c["stats"][u], p["toff"], p["tscale"])
    c["negated"] = ("v" if flip_v else "u") if negate else None
    c["table"] = dict(shape=shape, kind=TABLE_KINDS[(seed + seed // 7) % 3],
                      seed=int(rng.integers(1, 1 << 20)))
    c["knobs"] = dict(TF_KNOBS[(seed + seed // 4) % 4])
    return c


def tf_case(seed):
    """a whole frame from a baked plane under a 1-D table (k_march_plane_tf).  Dealt
    by the seed: the family (FAMILIES), within it the method (every one in turn), the
    dtype and the bin count or K; the table's size (TF_SIZES) and kind (TABLE_KINDS);
    the knobs (TF_KNOBS); one seed in four an edge shape, one in eight a negated
    window, one in 24 a 1 x 1 frame with the eye inside the volume.  Drawn: the
    other dims, frame, view, query state, window, table seed."""
    rng = np.random.default_rng(9500 + seed)
    family, turn = _turn(seed)
    u = TF_METHODS[family][turn % len(TF_METHODS[family])]
    c = dict(sweep="tf", seed=seed, u=u, v=None, **_tf_volume(rng, seed, family, turn, (u,)))
    return _tf_rest(rng, seed, c, u, None, 96, 72)


def _tf2_pair(family, turn):
    """(u, v) of a 2-D case: the four (CU, CV) instances in turn -- neither axis
    method 13, only u, only v, both (a codec volume has no method 13) -- the other
    methods in turn, u == v (one plane, bound twice) every fifth time"""
    if family == "codec":
        return 4 + turn % 3, 4 + (turn + turn // 3) % 3
    rest = tuple(m for m in TF_METHODS[family] if m != 13)
    inst, j = turn % 4, turn // 4
    a = rest[j % len(rest)]
    b = a if j % 5 == 4 else rest[(j + 1 + j // 3) % len(rest)]
    return ((a, b), (13, a), (a, 13), (13, 13))[inst]


def tf2_case(seed):
    """a whole frame from two baked planes under a 2-D table (k_march_tf2): tf_case's
    deals with the pair of _tf2_pair, the table's shape (TF2_SHAPES) and v's window
    by draw_window; every second negated window is v's"""
    rng = np.random.default_rng(10000 + seed)
    family, turn = _turn(seed)
    u, v = _tf2_pair(family, turn)
    c = dict(sweep="tf2", seed=seed, u=u, v=v, **_tf_volume(rng, seed, family, turn, (u, v)))
    return _tf_rest(rng, seed, c, u, v, 96, 72)


def tf_tile_case(seed):
    """a frame under a 1-D (even seeds) or a 2-D table split over 2-8 ranks' tile
    lists; the methods are drawn"""
    rng = np.random.default_rng(10500 + seed)
    family, turn = _turn(seed)
    methods = TF_METHODS[family]
    u = int(methods[int(rng.integers(0, len(methods)))])
    v = int(methods[int(rng.integers(0, len(methods)))]) if seed % 2 else None
    c = dict(sweep="tftiles", seed=seed, u=u, v=v, world=2 + seed % 7,
             **_tf_volume(rng, seed, family, turn, (u,) if v is None else (u, v)))
    return _tf_rest(rng, seed, c, u, v, 200, 120)


SWEEPS = {"hist": (hist_query_case, 96), "tiles": (hist_tile_case, 24), "f16": (f16_case, 48),
          "gmm": (gmm_case, 40), "chain": (gmm_chain_case, 16),
          "tf": (tf_case, 56), "tf2": (tf2_case, 72), "tftiles": (tf_tile_case, 16)}
TF_SWEEPS = ("tf", "tf2", "tftiles")


# ---- lit frames, gradient planes, ranges and histograms (tests/test_gpu_random_shading.py,
# tests/test_gpu_random_planes.py and the CPU census tests/test_random_planes.py) ----

GRADIENT = 32   # VR_QUERY_GRADIENT: method 32 + m is the gradient-magnitude plane of method m

# Nominal range of the gradient magnitude of each source statistic, for draw_window: not a
# bound.  Derived on the CPU from the reference planes of the lit sweeps' own volumes:
# ref_gradient.gradient_plane of the tf_plane of every record and codec case of lit_case
# (48 seeds) and lit_tile_case (8 seeds) whatever plane the case was dealt, the 90th
# percentile of the finite magnitudes per case, the median of those over the cases of a
# statistic, rounded to two digits (tests/test_random_planes.py::test_gradient_spans
# recomputes them and holds each entry within a factor of two).
SPAN.update({"grad mean": (0.0, 3.1), "grad variance": (0.0, 17.0), "grad entropy": (0.0, 6.0),
             "grad weights": (0.0, 11.0), "grad range": (0.0, 2.3), "grad quantile": (0.0, 2.5),
             "grad spread": (0.0, 2.9), "grad distance": (0.0, 4.1), "grad crossing": (0.0, 2.0)})

# (ka, kd, ks, k), k the exponent's log2, dealt by seed % 24: a matte light, diffuse only
# (ambient 0), a highlight of every exponent 2^0 .. 2^7, ks > 0 with kd = 0, the identity
# (once in 24: twice in lit_case's 48), coefficients that sum above 1 (colours saturate),
# and more of the same kinds
IDENTITY_LIGHT = (1.0, 0.0, 0.0, 0)
LIT_LIGHTS = ((0.3, 0.7, 0.0, 0), (0.0, 1.0, 0.0, 0), (0.2, 0.5, 0.6, 0), (0.2, 0.5, 0.6, 1),
              (0.1, 0.6, 0.5, 2), (0.3, 0.4, 0.5, 3), (0.2, 0.5, 0.6, 4), (0.0, 0.7, 0.6, 5),
              (0.25, 0.5, 0.5, 6), (0.0, 1.0, 1.0, 7), (0.4, 0.0, 0.8, 3), IDENTITY_LIGHT,
              (0.8, 0.9, 0.7, 2), (0.5, 0.5, 0.0, 0), (0.0, 0.0, 1.0, 1), (0.6, 0.4, 0.3, 5),
              (0.0, 0.25, 0.75, 0), (0.1, 0.9, 0.0, 0), (1.5, 0.5, 0.25, 6), (0.3, 0.0, 0.7, 7),
              (0.15, 0.35, 0.5, 4), (0.05, 2.0, 0.0, 0), (0.2, 0.3, 0.5, 2), (0.45, 0.55, 1.0, 1))


def _lit_gradient(family, turn):
    """whether a lit case marches the gradient plane of its method: 12 record cases in
    28 turns, shifted each round of the seven methods so that every method's gradient
    plane occurs, 4 codec cases in 8 (methods 5, 4, 6, 4), never a GMM volume"""
    if family == "records":
        return (turn + turn // 7) % 7 in (1, 3, 5)
    return family == "codec" and turn % 8 in (1, 3, 5, 6)


def _lit_case(rng, seed, sweep, u, grad, light, wmax, hmax, **more):
    family, turn = _turn(seed)
    c = dict(sweep=sweep, seed=seed, u=u, v=None, **more,
             **_tf_volume(rng, seed, family, turn, (u,)))
    plane = GRADIENT + u if grad else u
    if grad:
        c["stats"][plane] = "grad " + c["stats"][u]
    c = _tf_rest(rng, seed, c, plane, None, wmax, hmax)
    if seed % 4 == 2:
        c["table"] = None   # the built-in nine entries
    c.update(plane=plane, grad=grad, light=light)
    return c


def lit_case(seed):
    """a whole frame from a baked plane under a 1-D table and the headlight
    (k_march_lit).  tf_case's deals -- family, method, dtype, bins or K, edge shapes,
    table size and kind, negated window, the 1 x 1 frame seen from inside, TF_KNOBS -- and
    dealt besides: the plane (the method's own or, _lit_gradient, 32 + method), no
    table (the built-in nine) for one seed in four, the light (LIT_LIGHTS)"""
    rng = np.random.default_rng(11000 + seed)
    family, turn = _turn(seed)
    u = TF_METHODS[family][turn % len(TF_METHODS[family])]
    return _lit_case(rng, seed, "lit", u, _lit_gradient(family, turn), LIT_LIGHTS[seed % 24],
                     96, 72)


def lit_tile_case(seed):
    """a lit frame split over 2-8 ranks' tile lists; the method is drawn, the gradient
    plane dealt to seeds 1 (codec), 4 and 7 (records), the lights are LIT_LIGHTS[1::3]"""
    rng = np.random.default_rng(11500 + seed)
    family, _ = _turn(seed)
    methods = TF_METHODS[family]
    u = int(methods[int(rng.integers(0, len(methods)))])
    grad = family != "gmm" and seed % 3 == 1
    return _lit_case(rng, seed, "littiles", u, grad, LIT_LIGHTS[(3 * seed + 1) % 24], 200, 120,
                     world=2 + seed % 7)


# the sizes at which k_bake_grad's tiles (60 voxels of x plus an apron, 16 rows, 64 slices
# read ahead four at a time) and the planes' bricks (15 voxels, 2 rows) begin and end
GRAD_NX = (1, 2, 15, 16, 17, 59, 60, 61, 62, 76, 121)
GRAD_NY = (1, 2, 3, 15, 16, 17, 18, 33)
GRAD_NZ = (1, 2, 3, 4, 5, 6, 63, 64, 65, 66, 128, 129)
PLANE_FAMILIES = (("records", "f32"), ("records", "f16"), ("codec", "f32"))
PLANE_METHODS = {"records": (1, 2, 3, 10, 11, 12, 13), "codec": (4, 5, 6)}


def _plane_volume(rng, seed, dims, family, dtype, nb, methods):
    """a record or codec volume with the query state of `methods`, in the form the table
    sweeps' helpers read (test_random_cases.tf_records, tf_plane)"""
    c = dict(seed=seed, family=family, dims=dims, dtype=dtype, nb=nb)
    c["queries"], c["stats"] = draw_axis_queries(rng, family, methods, nb, dims, dtype, 0)
    return c


def make_wide(fill, shape):
    """the float32 values a case's `fill` entry writes over a plane: signed, the
    magnitudes log-uniform in [2^-20, 2^20], one value in 16 a +0, -0 or a denormal of
    either sign; nonfinite: +inf, -inf and NaN at three voxels each (fewer in a plane of
    fewer voxels)"""
    rng = np.random.default_rng(fill["seed"])
    n = int(np.prod(shape))
    a = (np.exp2(rng.uniform(-20, 20, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    small = np.array([0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00012345],
                     np.uint32).view(np.float32)
    pick = rng.random(n) < 1 / 16
    a[pick] = small[rng.integers(0, small.size, int(pick.sum()))]
    if fill["nonfinite"]:
        where = rng.choice(n, min(n, 9), replace=False)
        a[where] = np.resize(np.array([np.inf, -np.inf, np.nan], np.float32), where.size)
    return a.reshape(shape)


def grad_case(seed):
    """one bake of a gradient-magnitude plane (k_bake_grad).  Everything is dealt: the
    dims from GRAD_NX / GRAD_NY / GRAD_NZ, the source over PLANE_FAMILIES (seed % 3) and
    the family's methods in turn, the bin count; seeds 3 mod 4 overwrite the source plane
    with make_wide's values, seeds 7 mod 8 of those plant +-inf and NaN"""
    rng = np.random.default_rng(12000 + seed)
    dims = (GRAD_NX[seed % 11], GRAD_NY[(seed + seed // 8) % 8],
            GRAD_NZ[(seed + 5 * (seed // 12)) % 12])
    family, dtype = PLANE_FAMILIES[seed % 3]
    methods = PLANE_METHODS[family]
    u = methods[(seed // 3) % len(methods)]
    nb = (4, 8, 2)[(seed // 3) % 3]
    c = dict(sweep="grad", u=u, v=None, **_plane_volume(rng, seed, dims, family, dtype, nb, (u,)))
    c["fill"] = None
    if seed % 4 == 3:
        c["fill"] = dict(seed=int(rng.integers(1, 1 << 20)), nonfinite=seed % 8 == 7)
    return c


BOX_KINDS = ("whole", "voxel", "x end", "x start", "odd row", "even row", "slice", "inside")
WINDOW_KINDS = ("full", "default", "drawn", "negated", "zero", "one bin")
# bin counts by the number of LDS copies they leave room for, R = 32, 16, 8, 4, 2, 1 (nu *
# nv in (..512], (512, 1024], .. (8192, 16384]): nu of a 1-D call, (nu, nv) of a 2-D one
STAT_BINS_1D = ((1, 9, 37, 512), (1024, 521, 1000, 600), (2048, 1031, 1500, 2000),
                (4096, 2049, 3001, 4000), (8192, 4097, 5003, 8000), (16384, 8193, 16381, 12000))
STAT_BINS_2D = (((1, 1), (16, 8), (4, 3), (32, 16)), ((32, 32), (64, 16), (31, 33), (256, 4)),
                ((64, 32), (128, 16), (45, 45), (1024, 2)),
                ((64, 64), (256, 16), (63, 65), (2, 2048)),
                ((128, 64), (256, 32), (90, 91), (4096, 2)),
                ((128, 128), (256, 64), (127, 129), (16384, 1)))
FULL_BINS_1D, FULL_BINS_2D = (1, 5, 9, 16), ((1, 1), (3, 2), (4, 4), (8, 2))
STAT_VOXELS = 200_000


def _span(rng, n):
    a = int(rng.integers(0, n))
    return a, int(rng.integers(a + 1, n + 1))


def _stat_box(rng, kind, dims, turn):
    """the box of a stat case: None for the whole volume, else (x0, x1, y0, y1, z0, z1)"""
    nx, ny, nz = dims
    (x0, x1), (y0, y1), (z0, z1) = (_span(rng, n) for n in dims)
    k = int(rng.integers(1, max(nx // 15, 1) + 1))
    if kind == "whole":
        return None
    if kind == "voxel":
        x1, y1, z1 = x0 + 1, y0 + 1, z0 + 1
    elif kind == "x end":   # at 15 k, 15 k + 1 and 15 k - 1 in turn; all rows and slices
        x1 = min(max(15 * k + (0, 1, -1)[turn % 3], 1), nx)
        x0, y0, y1, z0, z1 = int(rng.integers(0, x1)), 0, ny, 0, nz
    elif kind == "x start":  # at 15 k and 15 k + 1 in turn; all rows and slices
        x0 = min(15 * k + turn % 2, nx - 1)
        x1, y0, y1, z0, z1 = int(rng.integers(x0 + 1, nx + 1)), 0, ny, 0, nz
    elif kind in ("odd row", "even row"):
        y0 = 2 * int(rng.integers(0, (ny + 1) // 2))
        if kind == "odd row" and y0 + 1 < ny:
            y0 += 1
        elif kind == "odd row" and y0 > 0:
            y0 -= 1
        x0, x1, y1, z0, z1 = 0, nx, y0 + 1, 0, nz
    elif kind == "slice":
        x0, x1, y0, y1, z1 = 0, nx, 0, ny, z0 + 1
    return (x0, x1, y0, y1, z0, z1)


def _stat_window(rng, kind, stat, turn):
    """a window of a stat case: None (the library's default), (offset, scale), or a kind
    the test resolves on the plane it holds: ("one bin", side) puts every finite value
    below the window (side 0) or above it (1), ("full",) is the box's own range"""
    off, scale = draw_window(rng, stat)
    if kind == "default":
        return None
    if kind == "drawn":
        return (off, scale)
    if kind == "negated":
        return _negated(stat, off, scale)
    if kind == "zero":
        return (off, 0.0)
    return ("one bin", turn % 2) if kind == "one bin" else ("full",)


def stat_case(seed):
    """one volume, its planes u and v (v None: a 1-D call), a box, bin counts and
    windows for plane_range, plane_window and plane_histogram.  Everything that matters
    is dealt: odd seeds are 2-D calls; with j = seed // 2 the family is PLANE_FAMILIES[j %
    3], the class of LDS copies (j + j // 6) % 6 and its bin counts STAT_BINS[j // 6]; the
    planes are the family's methods in turn, as themselves and as gradient planes (1-D:
    every second; 2-D in turn (a, b), (a, gradient of a), (gradient of a, b), (a, a));
    the box kind is BOX_KINDS[(seed + seed // 8) % 8]; u's window kind turns through
    WINDOW_KINDS against the classes, v's is u's where that is `zero` or `one bin` (so
    that every voxel meets one bin) and one of the other four else; a `full` window of u
    comes with the few bins of FULL_BINS and the most slices the cap allows, so that it
    can leave every bin populated; j = 1 mod 4 injects
    special values into plane u and poisons the slots that are no voxel's home."""
    rng = np.random.default_rng(12500 + seed)
    form, j = seed % 2, seed // 2
    ix, iy, iz = seed % 11, (3 * seed + seed // 8) % 8, (5 * seed + seed // 12) % 12
    if j % 2 == 1 or j % 6 == 0:   # the most slices the cap allows
        iz = 11
    while GRAD_NX[ix] * GRAD_NY[iy] * GRAD_NZ[iz] > STAT_VOXELS:
        iz = (iz - 1) % 12
    dims = (GRAD_NX[ix], GRAD_NY[iy], GRAD_NZ[iz])
    family, dtype = PLANE_FAMILIES[j % 3]
    methods = PLANE_METHODS[family]
    t = j // 3
    a, b = methods[t % len(methods)], methods[(t + 1 + t // 4) % len(methods)]
    if form == 0:
        u, v = (GRADIENT + a if t % 2 else a), None
    else:
        u, v = ((a, b), (a, GRADIENT + a), (GRADIENT + a, b), (a, a))[t % 4]
    sources = tuple(dict.fromkeys(m % GRADIENT for m in (u, v) if m is not None))
    c = dict(sweep="stat", u=u, v=v,
             **_plane_volume(rng, seed, dims, family, dtype, (4, 8, 2)[t % 3], sources))
    for m in (u, v):
        if m is not None and m > GRADIENT:
            c["stats"][m] = "grad " + c["stats"][m - GRADIENT]
    cls, turn = (j + j // 6) % 6, j // 6
    ku = WINDOW_KINDS[(5 * j) % 6]
    c["nu"], c["nv"] = (STAT_BINS_1D[cls][turn], 1) if form == 0 else STAT_BINS_2D[cls][turn]
    if ku == "full":   # few enough bins for a linear window to populate them all
        cls = 0
        c["nu"], c["nv"] = (FULL_BINS_1D[turn], 1) if form == 0 else FULL_BINS_2D[turn]
    c["copies"] = 32 >> cls
    c["box_kind"] = BOX_KINDS[(seed + seed // 8) % 8]
    c["box"] = _stat_box(rng, c["box_kind"], dims, seed // 8)
    kv = ku if ku in ("zero", "one bin") else \
        ("default", "drawn", "negated", "full")[(j + turn) % 4]
    c["window_kinds"] = (ku, kv if form else None)
    c["wu"] = _stat_window(rng, ku, c["stats"][u], turn)
    c["wv"] = _stat_window(rng, kv, c["stats"][v], turn + 1) if form else None
    c["inject"] = int(rng.integers(1, 1 << 20)) if j % 4 == 1 else None
    return c


PLANE_SWEEPS = {"lit": (lit_case, 48), "littiles": (lit_tile_case, 8), "grad": (grad_case, 24),
                "stat": (stat_case, 48)}
