"""CPU census of the random query sweeps (tests/random_cases.py, run on the GPU by
tests/test_gpu_random_queries.py and tests/test_gpu_random_transfer.py): the
generators and the references only.  It keeps
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
  tf        56       0        1 |     10          43    14 |     14      17     35
  tf2       72       0        1 |     18          55    16 |     18      20     54
  tftiles   16       0        0 |      3          12     5 |      6       3      5

(opaque is a lower bound: the final opacity can be told from the float frame only
where alpha * brightness stays below 1.)  A transfer window drawn blindly, as
test_gpu_random.draw_params draws it, left 35 of 96 method-10 frames without a
nonzero pixel; random_cases.draw_params places the window on the statistic's range.

The last three sweeps are the table marches' (tests/test_gpu_random_transfer.py:
frames from baked planes under a user-defined 1-D or 2-D table).  Their references
are ref_transfer.render_plane and ref_transfer2.render_planes over the planes numpy
computes per voxel (tf_plane).  For them the census also counts, as printed by
test_table_frames_reach_what_they_are_for: cases with samples on a footprint the
volume's edge clamps; nonzero frames of a volume dealt an edge nx (2, 15, 16, 17, 31,
32) and ny (2, 3, 5); 1 x 1 frames whose ray takes samples; 1-D frames that differ in
RGBA8 from the same planes and window under the built-in rainbow; `wide` tables
(entries outside [0, 1]) with a ray whose alpha ends below its alpha under the
table's abs(), so that opacity fell along it; and, for the 2-D whole frames, how
many differ in RGBA8 from each argument-level mutant of their reference, out of
those where the mutant can matter -- row 0 repeated over all rows (nv >= 2), column 0
over all columns (nu >= 2), v's window replaced by u's (nv >= 2 and the windows
differ), the two blends exchanged (exactly one axis is method 13), the two planes
exchanged under the same windows and blends (u != v and the planes differ: a GMM
volume's 10 and 13 are one plane).  Each must reach half; a sweep whose frames do
not notice a mutant would not notice that bug in the kernel either.

  sweep    clamped edge-nx 1x1 | rainbow  fell | row 0  column 0  u's window  blends planes
  tf         51/56      13   3 |   55/55  4/18 |
  tf2        64/72      18   3 |         12/23 | 53/56     54/56       53/56   27/29  40/46
  tftiles    14/16       4   1 |           3/6 |
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
import ref_numpy
import ref_quantile
import ref_transfer
import ref_transfer2
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
    return ref_crossing.render_plane(record_plane(pkg, case, vol), case["W"], case["H"], m,
                                     blend=blend_of(case["method"]), **render_kw(case))


def blend_of(method):
    """what makes a sample of a plane's 8 corners: the crossing combine for method
    13's plane of F, the trilinear blend for every other"""
    return ref_crossing.combine if method == 13 else ref_crossing.trilinear


def record_plane(pkg, case, vol):
    """the plane of case["method"] on the records vol as numpy computes it, (nz, ny,
    nx) float32: what bake_stats (1/2/3), bake_weighted, bake_quantile, bake_distance
    and bake_crossing hold per voxel.  A float16 vol is widened first."""
    method, q = case["method"], case["query"]
    wide = np.asarray(vol).astype(np.float32)
    with np.errstate(all="ignore"):
        if method in (1, 2, 3):
            return ref_numpy.stat(wide, method - 1)
        if method == 10:
            return ref_weighted.lin_stat(wide, query_weights(pkg, case))
        if method == 11:
            return ref_quantile.quantile_stat(wide, quantile_arg(q))
        if method == 12:
            return ref_distance.distance_stat(wide, distance_target(case, vol), q["metric"],
                                              q["similarity"])
    assert method == 13
    return ref_crossing.cdf_plane(vol, query_weights(pkg, case))


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


# ---- frames from baked planes under a table (random_cases.tf_case and the like) ----

def axis_case(case, method):
    """a table case as the helpers of one method read it: `method` and its `query`"""
    return dict(case, method=method, query=case["queries"].get(method, {}))


def tf_methods(case):
    return (case["u"],) if case["v"] is None else (case["u"], case["v"])


def tf_records(orc, case):
    """the family's records: hist_volume's, synth_codec's triple or gmm_records' pair"""
    if case["family"] == "records":
        return hist_volume(orc, case)
    if case["family"] == "codec":
        return orc.synth_codec(*case["dims"], case["nb"], seed=case["seed"])
    return gmm_records(orc, case)


def gmm_oracle_plane(orc, wide, method):
    """the oracle's mean (method 1) or variance statistic (2) of every voxel.  The
    census only: the library's planes meet these within 1e-4, not bit for bit."""
    wm, sg = wide
    flat_wm, flat_sg = wm.reshape(-1, *wm.shape[-2:]), sg.reshape(-1, sg.shape[-1])
    out = np.array([orc.gmm_stat(a, b, method) for a, b in zip(flat_wm, flat_sg)], np.float32)
    return out.reshape(sg.shape[:-1])


def tf_plane(pkg, orc, case, method, records):
    """the baked plane of `method` of a table case as numpy computes it, (nz, ny, nx)
    float32: record_plane for record volumes, ref_numpy's codec statistics of the
    decoded records, ref_gmm_range and ref_gmm_quantile per voxel for a GMM volume's
    queries (10 and 13 are both the range plane), the oracle for its mean and
    variance"""
    if case["family"] == "records":
        return record_plane(pkg, axis_case(case, method), records)
    with np.errstate(all="ignore"):
        if case["family"] == "codec":
            return ref_numpy.codec_stat(ref_numpy.codec_decode(*records), method - 4)
        wm, sg = records[1]
        table, steps = gmm_consts(pkg)
        q = case["queries"].get(method)
        if method == 10:
            return ref_gmm_range.range_stat(wm, sg, q["lo"], q["hi"], table)
        if method == 13:
            return ref_gmm_range.range_stat(wm, sg, -math.inf, q["theta"], table)
        if method == 11:
            spread = q["state"] == "spread"
            lo, hi = (q["lo"], q["hi"]) if spread else (q["q"], q["q"])
            return ref_gmm_quantile.quantile_stat(wm, sg, lo, hi, spread, table, steps)
    return gmm_oracle_plane(orc, records[1], method)


def tf_planes(pkg, orc, case, records=None):
    """{method: plane} of the case's axes"""
    records = tf_records(orc, case) if records is None else records
    return {mth: tf_plane(pkg, orc, case, mth, records) for mth in dict.fromkeys(tf_methods(case))}


def tf_reference(case, planes, m, table=None, info=None, swap_blends=False, swap_planes=False,
                 v_window=None, rainbow=False):
    """(RGBA8, float RGBA, samples) of a table case over `planes`: ref_transfer's frame
    for a 1-D table, ref_transfer2's for a 2-D one.  The other arguments are the
    census's mutants: another table, the blends or the planes of the two axes
    exchanged, another window for v, the built-in rainbow for a 1-D table."""
    W, H, u, v, kw = case["W"], case["H"], case["u"], case["v"], render_kw(case)
    table = rc.make_table(case["table"]) if table is None else table
    if v is None:
        if rainbow:
            return ref_crossing.render_plane(planes[u], W, H, m, blend=blend_of(u), info=info, **kw)
        return ref_transfer.render_plane(planes[u], W, H, m, table, blend=blend_of(u), info=info,
                                         **kw)
    pu, pv = (planes[v], planes[u]) if swap_planes else (planes[u], planes[v])
    bu, bv = (blend_of(v), blend_of(u)) if swap_blends else (blend_of(u), blend_of(v))
    voff, vscale = (case["voff"], case["vscale"]) if v_window is None else v_window
    return ref_transfer2.render_planes(pu, pv, W, H, m, table, blend_u=bu, blend_v=bv, voff=voff,
                                       vscale=vscale, info=info, **kw)


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


def table_census(case, m, planes, ref, info):
    """what a table case's reference adds to frame_census: samples on a clamped
    footprint; for a whole frame with a nonzero pixel whether it differs in RGBA8
    from the frame under the built-in rainbow (1-D) and from each argument-level
    mutant of ref_transfer2.render_planes that can matter for the case (None where
    it cannot), and for a `wide` table whether some ray's alpha ends below its alpha
    under the table's abs(): opacity fell along it"""
    u, v, nonzero = case["u"], case["v"], bool(np.any(ref[0] != 0))
    row = dict(clamped=info["clamped"] > 0, edge_nonzero=case["edge"] and nonzero, rainbow=None,
               tiny_hit=ref[2].shape == (1, 1) and bool(ref[2][0, 0] > 0),
               fell=None, mutants={k: None for k in MUTANTS})
    if not nonzero:
        return row
    table = rc.make_table(case["table"])
    differs = lambda **kw: bool(np.any(tf_reference(case, planes, m, **kw)[0] != ref[0]))
    if case["table"]["kind"] == "wide":
        plain = tf_reference(case, planes, m, table=np.abs(table))
        row["fell"] = bool(np.any((ref[2] >= 0) & (ref[1][..., 3] < plain[1][..., 3])))
    if case["sweep"] == "tftiles":  # (the larger frames: the whole-frame sweeps hold the rest)
        return row
    if v is None:
        row["rainbow"] = differs(rainbow=True)
        return row
    nv, nu = table.shape[:2]
    window = (case["params"]["toff"], case["params"]["tscale"])
    can = {"row 0": nv >= 2, "column 0": nu >= 2,
           "u's window": nv >= 2 and window != (case["voff"], case["vscale"]),
           "blends": (u == 13) != (v == 13),
           "planes": u != v and not np.array_equal(planes[u], planes[v], equal_nan=True)}
    args = {"row 0": dict(table=np.repeat(table[:1], nv, axis=0)),
            "column 0": dict(table=np.repeat(table[:, :1], nu, axis=1)),
            "u's window": dict(v_window=window), "blends": dict(swap_blends=True),
            "planes": dict(swap_planes=True)}
    for k in MUTANTS:
        if can[k]:
            row["mutants"][k] = differs(**args[k])
    return row


def reference_frame(pkg, orc, case, extra=None):
    """(camera, (RGBA8, float RGBA, samples)) of a case; extra: a dict that receives a
    table case's table_census"""
    m = camera(pkg, case)
    if case["sweep"] in rc.TF_SWEEPS:
        planes, info = tf_planes(pkg, orc, case), {}
        ref = tf_reference(case, planes, m, info=info)
        if extra is not None:
            extra.update(table_census(case, m, planes, ref, info))
        return m, ref
    if case["sweep"] in ("hist", "tiles"):
        return m, hist_reference_by_plane(pkg, case, hist_volume(orc, case), m)
    if case["sweep"] == "f16":
        return m, f16_reference(orc, case, hist_volume(orc, case), m)
    r = gmm_reference(pkg, orc, case, gmm_records(orc, case)[1], m)
    return m, (r["out"], r["out_f"], r["out_n"])


TYPES = ("opaque", "unsaturated", "short", "inside", "quarter", "narrow")
# the seeds whose reference frames the census renders (all of them where that is quick)
CENSUS_SEEDS = {"hist": range(96), "tiles": range(24), "f16": range(48), "gmm": range(40),
                "chain": range(16), "tf": range(56), "tf2": range(72), "tftiles": range(16)}
# the argument-level mutants of a 2-D frame's reference (table_census)
MUTANTS = ("row 0", "column 0", "u's window", "blends", "planes")


@functools.lru_cache(maxsize=None)
def census(pkg, orc, sweep):
    """one row per seed (computed once per sweep: two tests read the table sweeps')"""
    rows = []
    for seed in CENSUS_SEEDS[sweep]:
        case = make_case(pkg, sweep, seed)
        if not case.get("supported", True):
            rows.append(None)  # the library refuses the query: no frame
            continue
        extra = {}
        m, ref = reference_frame(pkg, orc, case, extra)
        rows.append(dict(frame_census(case, m, *ref), case=case, **extra))
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


@pytest.mark.parametrize("sweep", rc.TF_SWEEPS)
def test_table_frames_reach_what_they_are_for(pkg, orc, sweep):
    """the table sweeps, by the reference alone: at least one case in four takes
    samples on a clamped footprint and at least four nonzero frames come from an edge
    nx; three 1-D frames in four differ from the frame under the built-in rainbow;
    every mutant of a 2-D frame's reference changes at least half of the frames where
    it can; opacity falls along a ray of at least two `wide` frames; the ray of at
    least two 1 x 1 frames (one of the tile sweep's) takes samples"""
    rows = census(pkg, orc, sweep)
    share = lambda flags: (sum(flags), len(flags))
    clamped = sum(r["clamped"] for r in rows)
    edge = sum(r["edge_nonzero"] for r in rows)
    rainbow = share([r["rainbow"] for r in rows if r["rainbow"] is not None])
    fell = share([r["fell"] for r in rows if r["fell"] is not None])
    mutants = {k: share([r["mutants"][k] for r in rows if r["mutants"][k] is not None])
               for k in MUTANTS}
    tiny = sum(r["tiny_hit"] for r in rows)
    print(f"{sweep}: clamped {clamped}, edge nx nonzero {edge}, 1 x 1 hit {tiny}, differ from "
          f"the rainbow {rainbow[0]}/{rainbow[1]}, opacity fell {fell[0]}/{fell[1]}, mutants "
          + ", ".join(f"{k} {a}/{b}" for k, (a, b) in mutants.items()))
    assert 4 * clamped >= len(rows), (sweep, clamped)
    assert edge >= 4, (sweep, edge)
    assert tiny >= (1 if sweep == "tftiles" else 2), (sweep, tiny)
    if sweep == "tf":
        assert rainbow[1] >= 28 and 4 * rainbow[0] >= 3 * rainbow[1], rainbow
    if sweep == "tf2":
        for k, (a, b) in mutants.items():
            assert b >= 8 and 2 * a >= b, (k, a, b)
    assert fell[0] >= 2, fell


def _count(cases, **want):
    return sum(all(c.get(k) == v for k, v in want.items()) for c in cases)


def _count_query(cases, **want):
    return sum(all(c["query"].get(k) == v for k, v in want.items()) for c in cases)


def _table_sweeps_deal_their_combinations(cases):
    """what random_cases deals to the table sweeps, guaranteed and not merely likely"""
    tf, tf2, tiles = cases["tf"], cases["tf2"], cases["tftiles"]
    for sweep in (tf, tf2, tiles):
        n = len(sweep)
        assert 2 * _count(sweep, family="records") > n
        assert 6 * _count(sweep, family="codec") >= n and 6 * _count(sweep, family="gmm") >= n
        for knobs in rc.TF_KNOBS:  # both index widths: VR_TF_WIDE set and not
            assert _count(sweep, knobs=knobs) >= 4, knobs
        assert _count(sweep, edge=True) * 4 >= n - 3
        assert _count(sweep, W=1, H=1, kind=2) >= (2 if n > 24 else 1)
        assert {c["dims"][0] for c in sweep if c["edge"]} <= set(rc.EDGE_NX)
        assert {c["dims"][1] for c in sweep if c["edge"]} <= set(rc.EDGE_NY)
        for kind in rc.TABLE_KINDS:
            assert sum(c["table"]["kind"] == kind for c in sweep) >= 2, kind
        for c in sweep:
            t = rc.make_table(c["table"])
            assert t.dtype == np.float32 and np.isfinite(t).all() and t.size <= 4 * 1024
            assert t.shape == tuple(c["table"]["shape"]) + (4,)
            assert set(c["stats"]) == set(tf_methods(c)) and set(c["queries"]) <= set(c["stats"])
            assert all(mth in rc.TF_METHODS[c["family"]] for mth in tf_methods(c)), c
            if c["family"] == "records":  # a pair (10, 13) holds both states
                assert set(c["queries"]) == {mth for mth in tf_methods(c) if mth >= 10}, c
    for sweep in (tf, tf2):
        assert {c["dims"][0] for c in sweep if c["edge"]} == set(rc.EDGE_NX)
        assert {c["dims"][1] for c in sweep if c["edge"]} == set(rc.EDGE_NY)
        assert all(_count(sweep, family=f, edge=True) >= 1 for f in rc.TF_METHODS)
        assert _count(sweep, negated="u") >= 2
        for dtype in ("f32", "f16"):
            assert _count(sweep, family="records", dtype=dtype) >= 2
            assert _count(sweep, family="gmm", dtype=dtype) >= 2
        for nb in rc.INSTANCE_BINS:
            assert _count(sweep, family="records", nb=nb) >= 2, nb
            assert _count(sweep, family="codec", nb=nb) >= 1, nb
        for K in (8, 16, 32):
            assert _count(sweep, K=K) >= 2, K
    for family, methods in rc.TF_METHODS.items():
        for u in methods:
            assert _count(tf, family=family, u=u) >= 2, (family, u)
    for n in rc.TF_SIZES:
        assert sum(c["table"]["shape"] == (n,) for c in tf) >= 2, n
    assert all(c["v"] is None for c in tf) and all(c["v"] is not None for c in tf2)
    for cu in (False, True):
        for cv in (False, True):
            assert sum((c["u"] == 13) == cu and (c["v"] == 13) == cv for c in tf2) >= 4, (cu, cv)
    assert sum(c["u"] == c["v"] for c in tf2) >= 2
    assert sum(c["u"] == c["v"] != 13 for c in tf2) >= 2   # one blended plane bound twice
    assert any(set(tf_methods(c)) == {10, 13} and c["family"] == "records" for c in tf2)
    for shape in rc.TF2_SHAPES:
        assert sum(c["table"]["shape"] == shape for c in tf2) >= 2, shape
    assert _count(tf2, negated="v") >= 2
    assert {c["world"] for c in tiles} >= set(range(2, 9))
    assert _count(tiles, v=None) == len(tiles) // 2


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
    _table_sweeps_deal_their_combinations(cases)
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
            assert 1 <= c["W"] <= (200 if sweep in ("tiles", "tftiles") else 96)
            assert 1 <= c["H"] <= (120 if sweep in ("tiles", "tftiles") else 72)
            # (a GMM volume of a table sweep may be dealt an edge nx of 31 or 32)
            assert max(c["dims"][1:]) <= (24 if "K" in c else 32) and min(c["dims"]) >= 2
            assert c["dims"][0] <= (24 if "K" in c and not c.get("edge") else 32)
            assert 0.005 <= c["params"]["density"] <= 0.5001
            if sweep == "chain":
                assert c["dims"][2] >= c["nslabs"]
            if sweep in rc.TF_SWEEPS:
                assert c == eval(repr(c), {"inf": math.inf})  # printable: a failure shows it whole
                for off, scale in ((c["params"]["toff"], c["params"]["tscale"]),
                                   (c.get("voff", 0.0), c.get("vscale", 1.0))):
                    assert math.isfinite(off) and math.isfinite(scale) and scale != 0


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
