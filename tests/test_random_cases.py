"""CPU census of the random query sweeps (tests/random_cases.py, run on the GPU by
tests/test_gpu_random_queries.py): the generators and the references only.  It keeps
the sweeps from going vacuous -- frames of nothing, or draws that never reach the
geometry they are there for -- and holds the helpers that turn a case dict into its
volume, camera and reference frame, which the GPU tests import.

The census as it stands, over every seed of every sweep (printed by
test_reference_frames_are_worth_comparing).  "refused": fp32 records of 3, 5, 7 or 31 bins, which
no query has an instance for -- the GPU case asserts VR_ERR_UNSUPPORTED; they have
no frame and are counted with the all-zero frames against the limit of 1 in 4.
The other columns count frames that hold at least one ray that ends by opacity,
one that leaves the box unsaturated, a hit pixel of 1 or 2 samples; cameras with
the eye inside the volume, exact quarter turns; frames with W < 64 or H < 4.

  sweep  cases refused all-zero | opaque unsaturated short | inside quarter narrow
  hist      96      17        2 |     16          53    17 |     21      21     47
  tiles     24       0        1 |      5          12     4 |      6       8     15
  f16       48       0        5 |      8          33    17 |      9      16     33
  gmm       40       0        0 |      5          29    13 |     11      10     29
  chain     16       0        0 |      2           8     4 |      9       2      8

(opaque is a lower bound: the final opacity can be told from the float frame only
where alpha * brightness stays below 1.)  A transfer window drawn blindly, as
test_gpu_random.draw_params draws it, left 35 of 96 method-10 frames without a
nonzero pixel; random_cases.draw_params places the window on the statistic's range.
"""
import functools
import math

import numpy as np
import pytest

import random_cases as rc
import ref_crossing
import ref_distance
import ref_gmm_quantile
import ref_gmm_range
import ref_quantile
import ref_weighted

f32 = np.float32


# ---- a case dict -> camera, volume, reference ----

def camera(pkg, case):
    return pkg.camera.display_inv_view(case["rotation"], case["translation"])


def direction_of(pkg):
    """random_cases.gmm_chain_case's `direction` argument"""
    return lambda rot, tr, W, H: pkg.slabs.march_direction(pkg.camera.display_inv_view(rot, tr),
                                                           W, H)


def make_case(pkg, sweep, seed):
    gen = rc.SWEEPS[sweep][0]
    return gen(seed, direction_of(pkg)) if sweep == "chain" else gen(seed)


def render_kw(case):
    return dict(case["params"])


def oracle_params(orc, case, m, **kw):
    p = case["params"]
    return orc.make_params(case["W"], case["H"], m, density=p["density"],
                           brightness=p["brightness"], transfer_offset=p["toff"],
                           transfer_scale=p["tscale"], query_method=case["method"], **kw)


def hist_volume(orc, case):
    """the records to upload: float32, or narrowed to float16"""
    v = orc.synth_volume(*case["dims"], case["nb"], seed=case["seed"])
    return v.astype(np.float16) if case["dtype"] == "f16" else v


def query_weights(pkg, case):
    """the weights of a method-10 or method-13 case"""
    q, nb = case["query"], case["nb"]
    if q["state"] == "weights":
        return ref_weighted.seeded_weights(nb, seed=q["wseed"])
    if q["state"] == "range":
        return pkg.range_weights(q["lo"], q["hi"], nb)
    return pkg.range_weights(0.0, q["theta"], nb)


def quantile_arg(q):
    return (q["lo"], q["hi"]) if q["state"] == "spread" else q["q"]


def distance_target(case, vol):
    q = case["query"]
    if q["state"] == "target":
        return np.array(q["target"], np.float32)
    return ref_distance.region_mean(vol, q["lo"], q["hi"])


def hist_reference(pkg, case, vol, m):
    """(RGBA8, float RGBA, samples) of a histogram query case by the feature's own
    numpy reference; a float16 vol is widened by the reference"""
    W, H, q, kw = case["W"], case["H"], case["query"], render_kw(case)
    if case["method"] == 10:
        return ref_weighted.render(vol, query_weights(pkg, case), W, H, m, **kw)
    if case["method"] == 11:
        return ref_quantile.render(vol, quantile_arg(q), W, H, m, **kw)
    if case["method"] == 12:
        return ref_distance.render(vol, distance_target(case, vol), q["metric"], q["similarity"],
                                   W, H, m, **kw)
    return ref_crossing.render(vol, query_weights(pkg, case), W, H, m, **kw)


def hist_reference_by_plane(pkg, case, vol, m):
    """the same frame, faster: the references apply their statistic to the 8 gathered
    records of every sample, voxel by voxel; here it is applied to every voxel once
    and the march gathers the results (ref_crossing's restated loop, held against
    ref_weighted.render bit for bit by tests/test_crossing.py).  Used where frames
    are large (tile lists) and by the census; test_plane_route_is_the_reference
    holds the two against each other."""
    W, H, q, kw = case["W"], case["H"], case["query"], render_kw(case)
    wide = np.asarray(vol).astype(np.float32)
    blend = ref_crossing.trilinear
    if case["method"] == 10:
        plane = ref_weighted.lin_stat(wide, query_weights(pkg, case))
    elif case["method"] == 11:
        plane = ref_quantile.quantile_stat(wide, quantile_arg(q))
    elif case["method"] == 12:
        plane = ref_distance.distance_stat(wide, distance_target(case, vol), q["metric"],
                                           q["similarity"])
    else:
        plane, blend = ref_crossing.cdf_plane(vol, query_weights(pkg, case)), ref_crossing.combine
    return ref_crossing.render_plane(plane, W, H, m, blend=blend, **kw)


def gmm_records(orc, case, z_base=0, nslices=None):
    """(records to upload, the fp32 records the references decode)"""
    wm, sg = orc.synth_gmm(*case["dims"], case["K"], seed=case["seed"], z_base=z_base,
                           nslices=nslices)
    if case["dtype"] == "f16":
        hwm, hsg = wm.astype(np.float16), sg.astype(np.float16)
        return (hwm, hsg), (hwm.astype(np.float32), hsg.astype(np.float32))
    return (wm, sg), (wm, sg)


@functools.lru_cache(maxsize=None)
def gmm_consts(pkg):
    return pkg.gmm_phi_table(), pkg.gmm_quantile_steps()


def gmm_reference(pkg, orc, case, wide, m):
    """the frame of a whole GMM volume as the dict oracle.render_gmm returns (out,
    out_f, out_n): the oracle for mean and variance, ref_gmm_range and
    ref_gmm_quantile for the queries, ref_crossing on the range plane for method 13"""
    wm, sg = wide
    W, H, q, kw = case["W"], case["H"], case["query"], render_kw(case)
    table, steps = gmm_consts(pkg)
    if case["what"] in ("mean", "variance"):
        return orc.render_gmm(wm, sg, case["dims"], oracle_params(orc, case, m))
    if case["what"] == "range":
        return ref_gmm_range.render(wm, sg, q["lo"], q["hi"], table, W, H, m, **kw)
    if case["what"] == "quantile":
        spread = q["state"] == "spread"
        lo, hi = (q["lo"], q["hi"]) if spread else (q["q"], q["q"])
        return ref_gmm_quantile.render(wm, sg, lo, hi, spread, table, steps, W, H, m, **kw)
    F = ref_gmm_range.range_stat(wm, sg, -math.inf, q["theta"], table)
    out, out_f, out_n = ref_crossing.render_plane(F, W, H, m, **kw)
    return {"out": out, "out_f": out_f, "out_n": out_n}


def f16_reference(orc, case, vol, m):
    wide = np.asarray(vol).astype(np.float32)
    return orc.render(wide, oracle_params(orc, case, m, m7_dims=case["m7"]))[:3]


# ---- the census ----

def eye_inside(m):
    return bool(np.all(np.abs(np.asarray(m, np.float32).reshape(3, 4)[:, 3]) < 1))


def frame_census(case, m, rgba8, rgba_f, n):
    """what one reference frame contributes.  A ray's final opacity is read back from
    the float frame, alpha * brightness saturated at 1: below 1 it tells on which
    side of the 0.95 cut the ray ended, with a margin for the product's rounding."""
    b = case["params"]["brightness"]
    a = rgba_f[..., 3]
    hit = n > 0
    return dict(nonzero=bool(np.any(rgba8 != 0)),
                opaque=bool(np.any(hit & (a < 1) & (a > 0.951 * b))),
                unsaturated=bool(np.any(hit & (a < 1) & (a < 0.949 * b))),
                short=bool(np.any((n == 1) | (n == 2))),
                inside=eye_inside(m), quarter=case["kind"] == 1,
                narrow=case["W"] < 64 or case["H"] < 4)


def reference_frame(pkg, orc, case):
    m = camera(pkg, case)
    if case["sweep"] in ("hist", "tiles"):
        return m, hist_reference_by_plane(pkg, case, hist_volume(orc, case), m)
    if case["sweep"] == "f16":
        return m, f16_reference(orc, case, hist_volume(orc, case), m)
    r = gmm_reference(pkg, orc, case, gmm_records(orc, case)[1], m)
    return m, (r["out"], r["out_f"], r["out_n"])


TYPES = ("opaque", "unsaturated", "short", "inside", "quarter", "narrow")
# the seeds whose reference frames the census renders (all of them where that is quick)
CENSUS_SEEDS = {"hist": range(96), "tiles": range(24), "f16": range(48), "gmm": range(40),
                "chain": range(16)}


def census(pkg, orc, sweep):
    rows = []
    for seed in CENSUS_SEEDS[sweep]:
        case = make_case(pkg, sweep, seed)
        if not case.get("supported", True):
            rows.append(None)  # the library refuses the query: no frame
            continue
        m, ref = reference_frame(pkg, orc, case)
        rows.append(frame_census(case, m, *ref))
    return rows


@pytest.mark.parametrize("sweep", list(rc.SWEEPS))
def test_reference_frames_are_worth_comparing(pkg, orc, sweep):
    """at most 1 case in 4 without a nonzero RGBA8 pixel in its reference frame (a
    case the library refuses has no frame, and counts as one of them); and every
    kind of ray and camera the sweep is there for occurs"""
    rows = census(pkg, orc, sweep)
    frames = [r for r in rows if r is not None]
    empty = sum(1 for r in rows if r is None or not r["nonzero"])
    counts = {t: sum(r[t] for r in frames) for t in TYPES}
    print(f"{sweep}: {len(rows)} cases, {len(rows) - len(frames)} refused, "
          f"{empty - (len(rows) - len(frames))} frames all zero, {counts}")
    assert 4 * empty <= len(rows), (sweep, empty, len(rows))
    for t in TYPES:
        assert counts[t] >= 1, (sweep, t)
    if sweep == "chain":
        assert counts["inside"] >= 4


def _count(cases, **want):
    return sum(all(c.get(k) == v for k, v in want.items()) for c in cases)


def _count_query(cases, **want):
    return sum(all(c["query"].get(k) == v for k, v in want.items()) for c in cases)


def test_every_combination_occurs_twice(pkg):
    """generators only, every seed of every sweep"""
    cases = {s: [make_case(pkg, s, seed) for seed in range(n)] for s, (_, n) in rc.SWEEPS.items()}
    hist = [c for c in cases["hist"] if c["supported"]]
    assert len(cases["hist"]) - len(hist) >= 2   # bin counts only the fp32 marches 1/2/3/7 take
    assert all(c["dtype"] == "f32" for c in cases["hist"] if not c["supported"])
    for method in (10, 11, 12, 13):
        for dtype in ("f32", "f16"):
            for baked in (False, True):
                assert _count(hist, method=method, dtype=dtype, baked=baked) >= 2, \
                    (method, dtype, baked)
    for nb in rc.INSTANCE_BINS:
        assert _count(hist, nb=nb, dtype="f32") >= 2 and _count(hist, nb=nb, dtype="f16") >= 2, nb
    for state in ("weights", "range", "spread", "target", "region", "isovalue"):
        assert _count_query(hist, state=state) >= 2, state
    single = [c for c in hist if c["query"].get("state") == "q"]
    assert sum(c["query"]["q"] in (0.0, 1.0) for c in single) >= 2
    assert sum(0 < c["query"]["q"] < 1 for c in single) >= 2
    for metric in rc.METRICS:
        for sim in (False, True):
            assert _count_query(hist, metric=metric, similarity=sim) >= 2, (metric, sim)
    for knobs in rc.KNOBS:
        for s in cases:
            assert _count(cases[s], knobs=knobs) >= 2, (s, knobs)
    tiles = cases["tiles"]
    for method in (10, 11, 12, 13):
        assert _count(tiles, method=method) >= 2, method
    for key, values in (("dtype", ("f32", "f16")), ("baked", (False, True))):
        for v in values:
            assert _count(tiles, **{key: v}) >= 2, (key, v)
    assert {c["world"] for c in tiles} >= set(range(2, 9))
    half = cases["f16"]
    for method in (1, 2, 3):
        for baked in (False, True):
            assert _count(half, method=method, baked=baked) >= 2, (method, baked)
    assert _count(half, method=7, baked=True) >= 2 and _count(half, method=7, baked=False) == 0
    for nb in rc.INSTANCE_BINS:
        assert _count(half, nb=nb) >= 2, nb
    gmm = cases["gmm"]
    for K in (8, 16, 32):
        for dtype in ("f32", "f16"):
            assert _count(gmm, K=K, dtype=dtype) >= 2, (K, dtype)
    for what in ("mean", "variance"):
        assert _count(gmm, what=what, dtype="f16") >= 2 and _count(gmm, what=what, dtype="f32") == 0
    for what in ("range", "quantile"):
        for dtype in ("f32", "f16"):
            assert _count(gmm, what=what, dtype=dtype) >= 2, (what, dtype)
        for baked in (False, True):
            assert _count(gmm, what=what, baked=baked) >= 2, (what, baked)
    assert _count(gmm, what="crossing", baked=True) >= 2
    assert _count(gmm, what="crossing", baked=False) == 0
    ranges = [c["query"] for c in gmm if c["what"] == "range"]
    assert any(q["lo"] == -math.inf for q in ranges) and any(q["hi"] == math.inf for q in ranges)
    assert sum(math.isfinite(q["lo"]) and math.isfinite(q["hi"]) for q in ranges) >= 2
    for state in ("q", "spread"):
        assert _count_query([c for c in gmm if c["what"] == "quantile"], state=state) >= 2, state
    chain = cases["chain"]
    for nslabs in (2, 3, 4):
        assert _count(chain, nslabs=nslabs) >= 2, nslabs
    for dtype in ("f32", "f16"):
        assert _count(chain, dtype=dtype) >= 2, dtype
    for what in ("mean", "variance", "range", "quantile"):
        assert _count(chain, what=what) >= 2, what
    assert all(c["redraws"] <= rc.CHAIN_REDRAWS for c in chain)
    assert all(direction_of(pkg)(c["rotation"], c["translation"], c["W"], c["H"]) != 0
               for c in chain)


def test_cases_are_reproducible_and_in_bounds(pkg):
    for sweep, (_, n) in rc.SWEEPS.items():
        for seed in range(n):
            c = make_case(pkg, sweep, seed)
            assert c == make_case(pkg, sweep, seed)
            assert 1 <= c["W"] <= (200 if sweep == "tiles" else 96)
            assert 1 <= c["H"] <= (120 if sweep == "tiles" else 72)
            assert max(c["dims"]) <= (24 if "K" in c else 32) and min(c["dims"]) >= 2
            assert 0.005 <= c["params"]["density"] <= 0.5001
            if sweep == "chain":
                assert c["dims"][2] >= c["nslabs"]


@pytest.mark.parametrize("seed", (0, 1, 2, 3))
def test_plane_route_is_the_reference(pkg, orc, seed):
    """the statistic taken voxel by voxel and marched as a plane gives the frame of
    the feature's own reference bit for bit: one supported case of every method"""
    method = 10 + seed
    case = next(c for c in (rc.hist_query_case(s) for s in range(96))
                if c["supported"] and c["method"] == method and c["W"] * c["H"] <= 2500
                and c["nb"] >= 4)
    m = camera(pkg, case)
    vol = hist_volume(orc, case)
    a, b = hist_reference(pkg, case, vol, m), hist_reference_by_plane(pkg, case, vol, m)
    assert (a[2] > 0).any(), case
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y), case


def test_draw_view_is_the_camera_stream_of_test_gpu_random(pkg):
    """test_gpu_random.draw_camera's draws, restated as they stood before the views
    moved to random_cases: the same matrices and the same stream afterwards"""
    def before(rng):
        kind = rng.integers(0, 4)
        if kind == 0:
            return pkg.camera.display_inv_view(
                (0.0, 0.0),
                (rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), -rng.uniform(1.2, 6.0)))
        if kind == 1:
            rx, ry = (float(rng.choice([0, 90, 180, 270])) for _ in range(2))
            return pkg.camera.display_inv_view((rx, ry), (0.0, 0.0, -rng.uniform(2.5, 5.0)))
        if kind == 2:
            return pkg.camera.display_inv_view(
                (rng.uniform(-180, 180), rng.uniform(-180, 180)),
                (rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)))
        return pkg.camera.display_inv_view(
            (rng.uniform(-180, 180), rng.uniform(-180, 180)),
            (rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), -rng.uniform(1.5, 6.0)))

    from test_gpu_random import draw_camera
    kinds = set()
    for seed in range(1000, 1200):
        a, b = np.random.default_rng(seed), np.random.default_rng(seed)
        for _ in range(3):  # a case draws dims, bins and a frame before its camera
            assert np.array_equal(a.integers(2, 41, 3), b.integers(2, 41, 3))
            want, got = before(a), draw_camera(pkg, b)
            assert want.dtype == got.dtype and np.array_equal(want, got), seed
            assert a.uniform() == b.uniform()
        kinds.add(rc.draw_view(np.random.default_rng(seed))[0])
    assert kinds == {0, 1, 2, 3}
