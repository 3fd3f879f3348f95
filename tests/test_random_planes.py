"""CPU census of the random sweeps of the lit frames, the gradient-magnitude planes and
the ranges and histograms of baked planes (random_cases.PLANE_SWEEPS: lit_case,
lit_tile_case, grad_case, stat_case; run on the GPU by tests/test_gpu_random_shading.py
and tests/test_gpu_random_planes.py): what tests/test_random_cases.py is to the older
sweeps.  The generators and the numpy references only (ref_shading, ref_gradient,
ref_histogram over the planes numpy computes per voxel, test_random_cases.tf_plane).  It
proves that what the issue of each kernel names is dealt -- by construction, not by
luck -- that the reference results are worth comparing, and that the sweeps would notice
each mutant of their reference; and it holds the helpers that turn a case dict into
planes, windows and expected results, which the GPU tests import.

The census as it stands (printed by the tests):

  lit       48 frames, none all zero, 44 with samples on a clamped footprint, 30 with
            samples where g2 > 0 is false, c < 1 in 5 679 584 of 6 186 637 samples, 2
            1 x 1 frames hit; frames changed by each mutant of the reference, of the
            nonzero frames where it can act: the light ignored 44/46, the gradient not
            scaled by the dims 42/46, k off by one 33/36, kd and ks exchanged 42/42,
            alpha lit 44/46, the source for its gradient plane 15/16
  littiles   8 frames, none all zero, 8 clamped, 8 with flat samples, c < 1 in 2 624 461
            of 3 250 158 samples, 1 1 x 1 frame hit (mutants: the whole-frame sweep's)
  grad      24 bakes: every mutant of ref_gradient changes all 23 planes of more than
            one voxel; the three planes with planted infinities and NaNs keep finite
            magnitudes beside the NaN ones
  stat      48 calls, 3 of them refused (an injected infinity in a plane whose window is
            its own range: no finite window), 22 with every voxel in one bin, 7 using
            more than half of their bins, 5 `full` windows populate every bin; results
            changed by the mutants of ref_histogram, of the cases where each can act:
            aprons 26/26, empty slots 35/35, nearest 23/27, swapped 8/14, dropped 18/28

The gradient planes' windows come from SPAN's "grad ..." entries, derived as
test_gradient_spans restates.  The lit census renders every seed of both sweeps (33 s
for the whole file; the table sweeps' census takes 55 s).
"""
import functools

import numpy as np
import pytest

import random_cases as rc
import ref_gradient
import ref_histogram as rh
import ref_shading
from test_random_cases import (blend_of, camera, frame_census, render_kw, tf_plane, tf_records)

f32 = np.float32
G = rc.GRADIENT


# ---- a case dict -> planes, windows, references ----

def make_case(sweep, seed):
    return rc.PLANE_SWEEPS[sweep][0](seed)


def case_methods(case):
    """the planes a case reads, gradient planes as 32 + m"""
    if case["sweep"] in ("lit", "littiles"):
        return (case["plane"],)
    return tuple(dict.fromkeys(m for m in (case["u"], case["v"]) if m is not None))


def source_methods(case):
    return tuple(dict.fromkeys(m % G for m in case_methods(case)))


def with_gradients(case, sources):
    """{method: plane} of the case's planes from {source method: plane}: a gradient
    plane is ref_gradient.gradient_plane of its source"""
    return {m: ref_gradient.gradient_plane(sources[m - G])[0] if m > G else sources[m]
            for m in case_methods(case)}


def numpy_sources(pkg, orc, case):
    """{source method: the plane numpy computes per voxel}"""
    records = tf_records(orc, case)
    return {m: tf_plane(pkg, orc, case, m, records) for m in source_methods(case)}


def lit_reference(case, planes, m, info=None, light=None, mutant=None, plane=None):
    """(RGBA8, float RGBA, samples) of a lit case over `planes`; light, mutant, plane:
    the census's mutants"""
    table = None if case["table"] is None else rc.make_table(case["table"])
    F = planes[case["plane"]] if plane is None else plane
    return ref_shading.render_plane(F, case["W"], case["H"], m, table,
                                    case["light"] if light is None else light,
                                    blend=blend_of(case["plane"]), info=info, mutant=mutant,
                                    **render_kw(case))


SPECIALS = (np.nan, np.inf, -np.inf, 0.0, -0.0, -1e30, 1e30)


def inject(seed, plane):
    """a copy of the plane with SPECIALS -- NaN, both infinities, both zeros and values
    outside any window -- at up to 70 seeded voxels"""
    rng = np.random.default_rng(seed)
    p = np.array(plane, np.float32)
    where = rng.choice(p.size, min(p.size, 70), replace=False)
    p.ravel()[where] = np.resize(np.array(SPECIALS, np.float32), where.size)
    return p


def resolve_window(w, plane, box):
    """the window of a stat case as plane_histogram takes it (None: the library's
    default) and as the reference does"""
    if w is None:
        return None, rh.window(plane, box)
    if w[0] == "full":
        w = rh.window(plane, box)
    elif w[0] == "one bin":
        s = rh.crop(plane, box)
        s = s[np.isfinite(s)]
        lo, hi = (float(s.min()), float(s.max())) if s.size else (0.0, 0.0)
        # below the window: x < 0 for every finite value; above it: x >= 2
        w = (float(f32(hi + max(1.0, abs(hi)))), 1.0) if w[1] == 0 else \
            (float(f32(lo - 2 * max(1.0, abs(lo)))), 1.0)
    return w, w


def box_voxels(case):
    nx, ny, nz = case["dims"]
    x0, x1, y0, y1, z0, z1 = case["box"] or (0, nx, 0, ny, 0, nz)
    return (x1 - x0) * (y1 - y0) * (z1 - z0)


def stat_windows(case, planes):
    """(u's window, v's) as plane_histogram takes them, (u's, v's) as the reference does"""
    u, v, box = case["u"], case["v"], case["box"]
    wu, wu_ref = resolve_window(case["wu"], planes[u], box)
    wv, wv_ref = (None, (0.0, 1.0)) if v is None else resolve_window(case["wv"], planes[v], box)
    return (wu, wv), (wu_ref, wv_ref)


def refused(ref_windows):
    """a window taken from the range of a plane that holds an infinity is not finite:
    the library refuses the call (VR_ERR_ARG) and counts nothing"""
    return not all(np.isfinite(w).all() for w in ref_windows)


def stat_expected(case, planes, mutant=None):
    """the counts ref_histogram expects of a stat case over the planes {method: (nz, ny,
    nx)}"""
    u, v = case["u"], case["v"]
    wu_ref, wv_ref = stat_windows(case, planes)[1]
    return rh.histogram(planes[u], case["nu"], wu_ref, None if v is None else planes[v],
                        case["nv"], wv_ref, case["box"], mutant=mutant)


# ---- the deals ----

def _cases(sweep):
    return [make_case(sweep, s) for s in range(rc.PLANE_SWEEPS[sweep][1])]


def test_plane_cases_are_reproducible_and_printable():
    import math
    assert not set(rc.PLANE_SWEEPS) & set(rc.SWEEPS)
    for sweep in rc.PLANE_SWEEPS:
        for seed, c in enumerate(_cases(sweep)):
            assert c == make_case(sweep, seed) and c["seed"] == seed and c["sweep"] == sweep
            assert c == eval(repr(c), {"inf": math.inf}), c


def test_lit_sweeps_deal_their_combinations():
    lit, tiles = _cases("lit"), _cases("littiles")
    assert len(lit) == 48 and len(tiles) == 8
    for c in lit + tiles:
        assert c["v"] is None and c["u"] in rc.TF_METHODS[c["family"]]
        assert c["plane"] == (G + c["u"] if c["grad"] else c["u"])
        assert not (c["grad"] and c["family"] == "gmm")
        assert c["stats"][c["plane"]] in rc.SPAN
        assert c["light"] in rc.LIT_LIGHTS
    # tf_case's deals
    for family, methods in rc.TF_METHODS.items():
        for u in methods:
            assert sum(c["family"] == family and c["u"] == u for c in lit) >= 1, (family, u)
        assert sum(c["family"] == family and c["edge"] for c in lit) >= 1
    assert {c["dims"][0] for c in lit if c["edge"]} == set(rc.EDGE_NX)
    assert {c["dims"][1] for c in lit if c["edge"]} == set(rc.EDGE_NY)
    assert sum((c["W"], c["H"], c["kind"]) == (1, 1, 2) for c in lit) >= 2
    assert sum(c["negated"] == "u" for c in lit) >= 4
    for knobs in rc.TF_KNOBS:
        assert sum(c["knobs"] == knobs for c in lit) >= 4, knobs
    for dtype in ("f32", "f16"):
        assert sum(c["dtype"] == dtype and c["family"] == "records" for c in lit) >= 2
        assert sum(c["dtype"] == dtype and c["family"] == "gmm" for c in lit) >= 2
    # the plane: the gradient plane in one case of three, at least two per family, and
    # the gradient plane of every method
    assert 3 * sum(c["grad"] for c in lit) == len(lit)
    for family in ("records", "codec"):
        assert sum(c["grad"] and c["family"] == family for c in lit) >= 2
        assert {c["u"] for c in lit if c["grad"] and c["family"] == family} \
            == set(rc.TF_METHODS[family])
    assert sum(c["grad"] for c in tiles) >= 2
    # the table: none in one case of four; every size and kind among the others
    assert 4 * sum(c["table"] is None for c in lit) == len(lit)
    tables = [c["table"] for c in lit if c["table"] is not None]
    assert {t["shape"][0] for t in tables} == set(rc.TF_SIZES)
    assert {t["kind"] for t in tables} == set(rc.TABLE_KINDS)
    assert any(c["table"] is None for c in tiles)
    # the light
    lights = rc.LIT_LIGHTS
    assert len(lights) == 24 and len(set(lights)) == 24
    assert [c["light"] for c in lit] == [lights[s % 24] for s in range(48)]
    assert sum(c["light"] == rc.IDENTITY_LIGHT for c in lit) == 2
    assert all(c["light"] != rc.IDENTITY_LIGHT for c in tiles)
    assert any(ka == 0 and kd > 0 and ks == 0 for ka, kd, ks, k in lights)   # diffuse only
    assert sum(ka == 0 for ka, kd, ks, k in lights) >= 2
    assert {k for ka, kd, ks, k in lights if ks > 0} == set(range(8))
    assert any(ks > 0 and kd == 0 for ka, kd, ks, k in lights)
    assert any(ka + kd + ks > 1 for ka, kd, ks, k in lights)
    assert all(min(ka, kd, ks) >= 0 and 0 <= k <= 7 for ka, kd, ks, k in lights)
    assert {c["world"] for c in tiles} >= set(range(2, 9))


def _tiles(n, tile):
    return (n + tile - 1) // tile


def test_grad_sweep_deals_its_combinations():
    cases = _cases("grad")
    assert len(cases) == 24
    for axis, values, tile in ((0, rc.GRAD_NX, 60), (1, rc.GRAD_NY, 16), (2, rc.GRAD_NZ, 64)):
        assert {c["dims"][axis] for c in cases} == set(values)
        assert sum(_tiles(c["dims"][axis], tile) > 2 for c in cases) >= 2, axis
    assert all(c["dims"][0] <= 121 and c["dims"][1] <= 33 and c["dims"][2] <= 129 for c in cases)
    for family, dtype in rc.PLANE_FAMILIES:
        mine = [c for c in cases if (c["family"], c["dtype"]) == (family, dtype)]
        assert len(mine) == 8
        assert {c["u"] for c in mine} == set(rc.PLANE_METHODS[family])
    assert {c["u"] for c in cases} == {1, 2, 3, 4, 5, 6, 10, 11, 12, 13}
    fills = [c["fill"] for c in cases if c["fill"] is not None]
    assert 4 * len(fills) == len(cases) and 8 * sum(f["nonfinite"] for f in fills) == len(cases)
    assert [c["seed"] for c in cases if c["fill"] and c["fill"]["nonfinite"]] == [7, 15, 23]
    for f in fills:
        a = rc.make_wide(f, (5, 33, 121))
        fin = a[np.isfinite(a)]
        big = np.abs(fin[np.abs(fin) >= 2.0 ** -20])
        assert a.dtype == np.float32 and big.max() <= 2.0 ** 20 and (fin < 0).any()
        assert big.min() < 2.0 ** -18 and big.max() > 2.0 ** 18
        bits = a.view(np.uint32)
        assert (bits == 0).any() and (bits == 0x80000000).any()
        assert ((fin != 0) & (np.abs(fin) < 2.0 ** -126)).any()   # denormals
        assert np.isfinite(a).all() != f["nonfinite"]
        if f["nonfinite"]:
            assert (np.isnan(a).sum(), np.isposinf(a).sum(), np.isneginf(a).sum()) == (3, 3, 3)


def test_stat_sweep_deals_its_combinations():
    cases = _cases("stat")
    assert len(cases) == 48
    one, two = [c for c in cases if c["v"] is None], [c for c in cases if c["v"] is not None]
    for c in cases:
        nx, ny, nz = c["dims"]
        assert nx in rc.GRAD_NX and ny in rc.GRAD_NY and nz in rc.GRAD_NZ
        assert nx * ny * nz <= rc.STAT_VOXELS
        assert all(m % G in rc.PLANE_METHODS[c["family"]] for m in case_methods(c))
        assert 1 <= c["nu"] * c["nv"] <= 16384 and (c["v"] is not None or c["nv"] == 1)
        bins = c["nu"] * c["nv"]
        copies = max(r for r in (1, 2, 4, 8, 16, 32) if r * bins * 4 <= 65536)
        assert copies == c["copies"], c
        if c["box"] is not None:
            x0, x1, y0, y1, z0, z1 = c["box"]
            assert 0 <= x0 < x1 <= nx and 0 <= y0 < y1 <= ny and 0 <= z0 < z1 <= nz, c
    assert {c["dims"][0] for c in cases} == set(rc.GRAD_NX)
    assert {c["dims"][1] for c in cases} == set(rc.GRAD_NY)
    for family, dtype in rc.PLANE_FAMILIES:
        for form in (one, two):
            assert sum((c["family"], c["dtype"]) == (family, dtype) for c in form) == 8
    # the planes
    assert sum(c["u"] == c["v"] for c in two) >= 3
    assert sum(c["u"] > G for c in cases) >= 4 and sum(c["v"] > G for c in two) >= 4
    assert sum(c["u"] > G for c in two) >= 4
    assert sum(c["v"] == G + c["u"] for c in two) >= 3
    # the boxes
    for kind in rc.BOX_KINDS:
        assert sum(c["box_kind"] == kind for c in cases) >= 3, kind
    for c in cases:
        nx, ny, nz = c["dims"]
        if c["box_kind"] == "whole":
            assert c["box"] is None
            continue
        x0, x1, y0, y1, z0, z1 = c["box"]
        if c["box_kind"] == "voxel":
            assert box_voxels(c) == 1
        elif c["box_kind"] == "x end":
            assert x1 == nx or x1 == 1 or x1 % 15 in (0, 1, 14), c
        elif c["box_kind"] == "x start":
            assert x0 == nx - 1 or x0 % 15 in (0, 1), c
        elif c["box_kind"] in ("odd row", "even row"):
            assert y1 == y0 + 1 and (y0 % 2 == (c["box_kind"] == "odd row") or ny == 1), c
        elif c["box_kind"] == "slice":
            assert (x0, x1, y0, y1, z1) == (0, nx, 0, ny, z0 + 1)
    ends = {c["box"][1] % 15 for c in cases if c["box_kind"] == "x end" and c["dims"][0] > 16
            and c["box"][1] < c["dims"][0]}
    starts = {c["box"][0] % 15 for c in cases if c["box_kind"] == "x start" and c["dims"][0] > 17}
    assert ends >= {0, 1, 14} and starts >= {0, 1}, (ends, starts)
    # the bin counts
    for form in (one, two):
        for copies in (32, 16, 8, 4, 2, 1):
            assert sum(c["copies"] == copies for c in form) >= 2, copies
    shapes = {(c["nu"], c["nv"]) for c in two}
    assert {(1, 1), (128, 128), (256, 64)} <= shapes
    assert any(c["nu"] == 16384 for c in one)
    assert any(c["nu"] > 2 and all(c["nu"] % d for d in range(2, int(c["nu"] ** 0.5) + 1))
               for c in one)
    # the windows
    for kind in rc.WINDOW_KINDS:
        assert sum(c["window_kinds"][0] == kind for c in cases) >= 4, kind
    assert sum(c["window_kinds"] == ("one bin", "one bin") for c in two) >= 2
    assert sum(c["wu"] is not None and len(c["wu"]) == 2 and c["wu"][1] < 0 for c in cases) >= 2
    assert sum(c["wu"] is not None and len(c["wu"]) == 2 and c["wu"][1] == 0 for c in cases) >= 2
    assert 4 * sum(c["inject"] is not None for c in cases) == len(cases)
    assert any(c["inject"] for c in one) and any(c["inject"] for c in two)


# ---- the lit frames ----

LIT_MUTANTS = ("no light", "unscaled", "k off by one", "kd and ks", "lit alpha", "source plane")


def lit_row(pkg, orc, case, mutants):
    """what one lit case's reference contributes to the census"""
    m = camera(pkg, case)
    planes = with_gradients(case, numpy_sources(pkg, orc, case))
    info = {}
    ref = lit_reference(case, planes, m, info=info)
    row = dict(frame_census(case, m, *ref), clamped=info["clamped"] > 0, flat=info["flat"] > 0,
               samples=info["samples"], below=int((info["c"] < 1).sum()),
               tiny_hit=ref[2].shape == (1, 1) and bool(ref[2][0, 0] > 0), mutants={}, case=case)
    if not (mutants and row["nonzero"]):
        return row
    ka, kd, ks, k = case["light"]
    lit = case["light"] != rc.IDENTITY_LIGHT
    trials = {"no light": (lit, dict(light=rc.IDENTITY_LIGHT)),
              "unscaled": (lit and len(set(case["dims"])) > 1, dict(mutant="unscaled")),
              "k off by one": (ks > 0, dict(light=(ka, kd, ks, k + 1 if k < 7 else k - 1))),
              "kd and ks": (kd != ks, dict(light=(ka, ks, kd, k))),
              "lit alpha": (lit, dict(mutant="lit_alpha")),
              "source plane": (case["grad"], dict(plane=numpy_sources(pkg, orc, case)[case["u"]])
                               if case["grad"] else {})}
    for name, (can, kw) in trials.items():
        if can:
            row["mutants"][name] = bool(np.any(lit_reference(case, planes, m, **kw)[0] != ref[0]))
    return row


@functools.lru_cache(maxsize=None)
def lit_census(pkg, orc, sweep):
    return [lit_row(pkg, orc, c, sweep == "lit") for c in _cases(sweep)]


@pytest.mark.parametrize("sweep", ("lit", "littiles"))
def test_lit_frames_are_worth_comparing(pkg, orc, sweep):
    rows = lit_census(pkg, orc, sweep)
    n = len(rows)
    empty = sum(not r["nonzero"] for r in rows)
    clamped, flat = sum(r["clamped"] for r in rows), sum(r["flat"] for r in rows)
    samples, below = sum(r["samples"] for r in rows), sum(r["below"] for r in rows)
    tiny = sum(r["tiny_hit"] for r in rows)
    share = {k: (sum(r["mutants"][k] for r in rows if k in r["mutants"]),
                 sum(k in r["mutants"] for r in rows)) for k in LIT_MUTANTS}
    print(f"{sweep}: {n} frames, {empty} all zero, clamped {clamped}, flat {flat}, c < 1 in "
          f"{below} of {samples} samples, 1 x 1 hit {tiny}, mutants "
          + ", ".join(f"{k} {a}/{b}" for k, (a, b) in share.items()))
    assert 4 * empty <= n, (sweep, empty)
    assert 4 * clamped >= n, (sweep, clamped)
    assert 2 * below >= samples > 0, (below, samples)
    if sweep == "lit":
        assert flat >= 4 and tiny >= 2, (flat, tiny)
        for k, (a, b) in share.items():
            assert b >= 8 and 2 * a >= b, (k, a, b)
    else:
        assert flat >= 1 and tiny >= 1, (flat, tiny)


def test_gradient_spans(pkg, orc):
    """SPAN's "grad ..." entries as their comment derives them: per statistic the median
    over the lit sweeps' record and codec cases of the 90th percentile of the gradient
    magnitude of the case's source plane; each entry within a factor of two of that"""
    per = {}
    for c in _cases("lit") + _cases("littiles"):
        if c["family"] == "gmm":
            continue
        mag = ref_gradient.gradient_plane(numpy_sources(pkg, orc, c)[c["u"]])[0]
        mag = mag[np.isfinite(mag)]  # (the entropy of one bin is NaN)
        if mag.size:
            per.setdefault("grad " + c["stats"][c["u"]], []).append(float(np.percentile(mag, 90)))
    got = {k: float(np.median(v)) for k, v in sorted(per.items())}
    print("gradient spans:", {k: f"{v:.2g}" for k, v in got.items()})
    assert set(got) == {k for k in rc.SPAN if k.startswith("grad ")}
    for k, v in got.items():
        a, b = rc.SPAN[k]
        assert a == 0 and b / 2 <= v <= b * 2, (k, v, b)


# ---- the gradient planes ----

def grad_source(pkg, orc, case):
    """the source plane of a grad case as numpy computes it, overwritten where the case
    says so"""
    if case["fill"] is not None:
        return rc.make_wide(case["fill"], case["dims"][::-1])
    return numpy_sources(pkg, orc, case)[case["u"]]


def _same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def test_gradient_cases_tell_every_mutant(pkg, orc):
    cases = _cases("grad")
    shown = 0
    for c in cases:
        s = grad_source(pkg, orc, c)
        assert s.shape == c["dims"][::-1] and s.dtype == np.float32
        with np.errstate(all="ignore"):
            right = ref_gradient.gradient_plane(s)[0]
            if max(c["dims"]) == 1:
                continue
            for mutant in ref_gradient.MUTANTS:  # each touches every axis of n > 1
                assert not _same_bits(ref_gradient.gradient_plane(s, mutant)[0], right), (mutant, c)
        shown += 1
        if c["fill"] is not None and c["fill"]["nonfinite"]:
            assert np.isnan(right).any() and np.isfinite(right).any(), c
    print(f"grad: {len(cases)} bakes, every mutant changes all {shown} planes of more than one "
          f"voxel")
    assert shown >= 20
    small = sorted(cases, key=lambda c: (int(np.prod(c["dims"])), c["seed"]))[:3]
    for c in small:
        s = grad_source(pkg, orc, c)
        with np.errstate(all="ignore"):
            a, amax = ref_gradient.gradient_plane(s)
            b, bmax = ref_gradient.gradient_plane_scalar(s)
        assert _same_bits(a, b) and _same_bits(amax, bmax), c


# ---- ranges and histograms ----

def stat_planes(pkg, orc, case):
    """{method: plane} of a stat case from numpy's planes, plane u injected where the
    case says so"""
    planes = with_gradients(case, numpy_sources(pkg, orc, case))
    if case["inject"] is not None:
        planes = dict(planes)
        planes[case["u"]] = inject(case["inject"], planes[case["u"]])
    return planes


def _can_act(case, mutant):
    nx, ny, nz = case["dims"]
    x0, x1, y0, y1, z0, z1 = case["box"] or (0, nx, 0, ny, 0, nz)
    ku, kv = case["window_kinds"]
    pinned = lambda k: k in ("zero", "one bin")
    if mutant == "aprons":
        return any(x > 0 and x % 15 == 0 for x in range(x0, x1))
    if mutant == "empty_slots":
        return rh._extra_slots((nz, ny, nx), case["box"], mutant)[1] > 0
    if mutant == "nearest":  # an axis of several bins whose window does not pin every value
        return (case["nu"] > 1 and not pinned(ku)) or (case["nv"] > 1 and not pinned(kv))
    if mutant == "swapped":
        return case["v"] is not None and case["u"] != case["v"] and box_voxels(case) > 1
    # dropped: a window that leaves values outside, or injected ones
    return case["inject"] is not None or any(k in ("drawn", "negated", "one bin") for k in (ku, kv))


def test_stat_cases_are_worth_running(pkg, orc):
    cases = _cases("stat")
    one_bin = spread = full = no_window = 0
    share = {k: [0, 0] for k in rh.MUTANTS}
    for c in cases:
        planes = stat_planes(pkg, orc, c)
        if refused(stat_windows(c, planes)[1]):
            assert c["inject"] is not None, c
            no_window += 1
            continue
        want = stat_expected(c, planes)
        assert want.shape == (c["nv"], c["nu"]) and int(want.sum()) == box_voxels(c), c
        one_bin += int(want.max()) == box_voxels(c)
        used = int(np.count_nonzero(want))
        spread += 2 * used > want.size
        full += c["window_kinds"][0] == "full" and used == want.size
        for k in rh.MUTANTS:
            if _can_act(c, k):
                share[k][1] += 1
                share[k][0] += not np.array_equal(stat_expected(c, planes, mutant=k), want)
    print(f"stat: {len(cases)} calls, {no_window} refused (no finite window), every voxel in "
          f"one bin {one_bin}, more than half of the "
          f"bins used {spread}, `full` windows with every bin populated {full}, mutants "
          + ", ".join(f"{k} {a}/{b}" for k, (a, b) in share.items()))
    assert one_bin >= 6 and spread >= 6 and full >= 4, (one_bin, spread, full)
    assert 1 <= no_window <= 4, no_window
    for k, (a, b) in share.items():
        assert b >= 6 and 2 * a >= b, (k, a, b)
