"""Pure case generators of the seeded random sweeps (tests/test_gpu_random.py,
tests/test_gpu_random_queries.py and the CPU census tests/test_random_cases.py).

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


def draw_params(rng, stat):
    """density, brightness and the transfer window for the statistic `stat`"""
    density = _f32(math.exp(rng.uniform(math.log(0.005), math.log(0.5))))
    brightness = _f32(rng.uniform(0.5, 2.0))
    blind = bool(rng.integers(0, 8) == 0)
    u, v = rng.uniform(), rng.uniform()
    if blind:
        toff, tscale = -0.2 + 0.4 * u, 0.5 + 1.5 * v
    else:
        a, b = SPAN[stat]
        tscale = (0.35 + 0.5 * v) / (b - a)
        toff = a - (0.08 + 0.17 * u) / tscale
    return dict(density=density, brightness=brightness, toff=_f32(toff), tscale=_f32(tscale))


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


SWEEPS = {"hist": (hist_query_case, 96), "tiles": (hist_tile_case, 24), "f16": (f16_case, 48),
          "gmm": (gmm_case, 40), "chain": (gmm_chain_case, 16)}
