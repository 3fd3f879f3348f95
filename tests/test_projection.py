"""The ray projections without a GPU: known answers of the
numpy march (tests/ref_projection.py), its scalar restatement, its tie to the
existing reference (the samples of a frame whose table is transparent everywhere),
the host state of the C ABI (vr_set_projection makes no device call), the reference
frames the GPU tests compare against, and the census of the seeded sweep of
tests/test_gpu_random_projection.py."""
import ctypes
import functools

import numpy as np
import pytest

import random_cases as rc
import ref_crossing
import ref_projection
import ref_transfer
from test_crossing import BAKE, DIMS, H, W, camera, cdf
from test_transfer import BLENDS, RAMP2, RAND256, TABLES

f32 = np.float32
MODES = ("max", "min", "mean")
VIEWS = ("C0", "C1", "S")


def frame(F, mode, cam="C1", blend="trilinear", table=None, info=None, **kw):
    return ref_projection.render_plane(F, W, H, camera(cam), mode, table, blend=BLENDS[blend],
                                       info=info, **kw)


# ---- known answers ----

@pytest.mark.parametrize("blend", sorted(BLENDS))
def test_constant_plane(blend):
    """every sample of a constant plane c is one value s (c for the trilinear blend:
    (1 - a) c + a c is exact for the 8-bit weights here; the combine's value of eight
    equal corners): MAX = MIN = s, MEAN = (s + ... + s) / n summed in the same order"""
    c = f32(0.3125)
    F = np.full(DIMS[::-1], c, np.float32)
    s = f32(BLENDS[blend](np.full((8,), c, np.float32), [(0, 0, f32(0.5))] * 3))
    if blend == "trilinear":
        assert s == c
    acc = {}
    for mode in MODES:
        info = {}
        n = frame(F, mode, blend=blend, info=info)[2]
        acc[mode] = info["acc"]
        hit = n >= 0
        assert hit.sum() == 1330 and n[hit].min() >= 1
    assert np.all(acc["max"][hit] == s) and np.all(acc["min"][hit] == s)
    want = np.zeros_like(acc["mean"])
    for y, x in zip(*np.nonzero(hit)):
        t = f32(0)
        for _ in range(n[y, x]):
            t = f32(t + s)
        want[y, x] = f32(t / f32(n[y, x]))
    assert np.array_equal(acc["mean"], want)


def test_one_voxel():
    """a plane that is 0 but for one voxel: MAX > 0 exactly on the rays some footprint
    of which touches the voxel, MIN is 0 on every ray that has a sample away from it"""
    F = np.zeros(DIMS[::-1], np.float32)
    vz, vy, vx = 8, 10, 12
    F[vz, vy, vx] = 1
    info = {}
    n = frame(F, "max", info=info)[2]
    hit = n >= 0
    # the rays near the voxel's image, one at a time (the others cannot reach it)
    ys, xs = np.nonzero(info["acc"] > 0)
    assert ys.size > 4
    box = np.zeros((H, W), bool)
    box[max(ys.min() - 2, 0):ys.max() + 3, max(xs.min() - 2, 0):xs.max() + 3] = True
    touched = np.zeros((H, W), bool)
    for y, x in zip(*np.nonzero(hit & box)):
        touched[y, x] = _touches(F.shape, camera("C1"), x, y, (vx, vy, vz))
    assert 0 < touched.sum() < (hit & box).sum()
    # (a footprint that touches the voxel with a zero weight gives a zero sample)
    assert not np.any((info["acc"] > 0) & ~touched)
    assert (info["acc"] > 0).sum() > touched.sum() // 2
    assert np.all(info["acc"][hit] >= 0) and info["acc"].max() <= 1
    assert np.all(info["acc"][hit & ~box] == 0)
    lo = {}
    frame(F, "min", info=lo)
    assert np.all(lo["acc"][hit & ~touched & (n > 1)] == 0)


def _touches(shape, m, x, y, voxel):
    """some footprint along the ray of pixel (x, y) has `voxel` among its 8 corners"""
    seen = []
    probe = np.zeros(shape, np.float32)
    probe[voxel[2], voxel[1], voxel[0]] = 1

    def blend(vals, ax):
        seen.append(bool(np.any(vals != 0)))
        return f32(0)
    ref_projection.render_ray(probe, W, H, m, x, y, "max", blend=blend)
    return any(seen)


def test_nan_voxels_are_skipped_by_max_and_min():
    rng = np.random.default_rng(2401)
    F = rng.random(DIMS[::-1]).astype(np.float32)
    holes = F.copy()
    holes[rng.random(F.shape) < 0.02] = np.nan
    for mode, fill in (("max", -np.inf), ("min", np.inf)):
        a, b = {}, {}
        n = frame(holes, mode, blend="trilinear", info=a)[2]
        hit = n >= 0
        assert not np.isnan(a["acc"][hit]).all()
        # the same frame by a march that replaces a NaN sample by the identity
        nanless = lambda v, ax, fill=fill: np.where(
            np.isnan(s := ref_crossing.trilinear(v, ax)), f32(fill), s).astype(np.float32)
        ref_projection.render_plane(holes, W, H, camera("C1"), mode, blend=nanless, info=b)
        assert np.array_equal(a["acc"], b["acc"])
        assert np.isfinite(a["acc"][hit]).sum() > hit.sum() // 2
    m = {}
    frame(holes, "mean", info=m)
    assert np.isnan(m["acc"][hit]).any()  # the mean keeps them: a sum has no skip


@pytest.mark.parametrize("blend", sorted(BLENDS))
@pytest.mark.parametrize("mode", MODES)
def test_scalar_loop_is_the_array_march(mode, blend):
    """20 seeded pixels, one ray at a time in Python scalars"""
    F, m = cdf(DIMS, 8, "f32"), camera("C1")
    info = {}
    rgba8, rgba, n = ref_projection.render_plane(F, W, H, m, mode, RAND256, blend=BLENDS[blend],
                                                 brightness=1.25, toff=0.05, tscale=1.5, info=info)
    rng = np.random.default_rng(2402)
    ys, xs = np.nonzero(n >= 0)
    pick = rng.choice(ys.size, 17, replace=False)
    pixels = [(int(xs[i]), int(ys[i])) for i in pick] + [(0, 0), (W - 1, H - 1), (W // 2, 0)]
    hits = 0
    for x, y in pixels:
        got, gn, acc = ref_projection.render_ray(F, W, H, m, x, y, mode, RAND256,
                                                 blend=BLENDS[blend], brightness=1.25, toff=0.05,
                                                 tscale=1.5)
        assert gn == n[y, x], (x, y)
        if gn < 0:
            continue
        hits += 1
        assert f32(acc).tobytes() == info["acc"][y, x].tobytes(), (x, y)
        assert got.tobytes() == rgba[y, x].tobytes(), (x, y)
    assert hits >= 17


# ---- the tie to the existing reference ----

@pytest.mark.parametrize("dims,nb", ((DIMS, 8), (BAKE, 4)), ids=("DIMS", "BAKE"))
def test_samples_are_those_of_a_transparent_frame(dims, nb):
    """no ray of a frame whose table has alpha 0 everywhere ends early, so its samples
    per pixel are the projection's, whatever the mode"""
    clear = RAND256.copy()
    clear[:, 3] = 0
    F = cdf(dims, nb, "f32")
    for cam in VIEWS:
        for blend in sorted(BLENDS):
            info = {}
            want = ref_transfer.render_plane(F, W, H, camera(cam), clear, blend=BLENDS[blend],
                                             info=info)[2]
            assert not info["early"].any()
            for mode in MODES:
                assert np.array_equal(frame(F, mode, cam, blend)[2], want), (cam, blend, mode)


# ---- the reference frames of the GPU tests ----

@functools.lru_cache(maxsize=None)
def reference(dims, nb, dtype, cam, w, h, table, blend, mode):
    """the numpy frame of the projection `mode` under TABLES[table] (None: the built-in
    table) with BLENDS[blend] over the plane of F of test_crossing.cdf, computed once
    per case and shared by the CPU and the GPU tests: (RGBA8, float RGBA, samples),
    arrays read-only"""
    ref = ref_projection.render_plane(cdf(dims, nb, dtype), w, h, camera(cam), mode,
                                      None if table is None else TABLES[table],
                                      blend=BLENDS[blend])
    for a in ref:
        a.setflags(write=False)
    return ref


# (view, blend, mode) -> (hit pixels, the longest ray, one-sample rays) of DIMS x 8 f32
# at 64 x 48: the rays are the view's alone
_RAYS = {"C0": (1389, 207, 56), "C1": (1330, 296, 11), "S": (1389, 207, 56)}
PINNED = {(cam, blend, mode): _RAYS[cam] for cam in VIEWS for blend in sorted(BLENDS)
          for mode in MODES}


@pytest.mark.parametrize("cam,blend", [(c, b) for c in VIEWS for b in sorted(BLENDS)])
def test_reference_frames_are_worth_comparing(cam, blend):
    """by the reference alone: the rays pinned, hit pixels of many colours, the three
    modes three frames, none of them the composited frame under the same table"""
    frames = {mode: reference(DIMS, 8, "f32", cam, W, H, "rand256", blend, mode) for mode in MODES}
    composited = ref_transfer.render_plane(cdf(DIMS, 8, "f32"), W, H, camera(cam), RAND256,
                                           blend=BLENDS[blend])
    for mode, (rgba8, _, n) in frames.items():
        hit = n >= 0
        colours = np.unique(rgba8[hit]).size
        print(cam, blend, mode, int(hit.sum()), int(n.max()), int((n == 1).sum()), colours)
        assert (int(hit.sum()), int(n.max()), int((n == 1).sum())) == PINNED[cam, blend, mode]
        assert colours > 40
        assert np.array_equal(hit, composited[2] >= 0)
        assert (rgba8 != composited[0]).sum() > 900
        small = reference(BAKE, 4, "f32", cam, W, H, "rand256", blend, mode)
        assert np.unique(small[0][small[2] >= 0]).size > 10
    for a, b in (("max", "min"), ("max", "mean"), ("min", "mean")):
        assert (frames[a][0] != frames[b][0]).sum() > 900, (a, b)


def test_no_table_is_the_reference_table(pkg):
    F = cdf(DIMS, 8, "f32")
    for mode in MODES:
        for blend in sorted(BLENDS):
            a = frame(F, mode, blend=blend)
            b = frame(F, mode, blend=blend, table=pkg.REFERENCE_TF)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)


# ---- host state of the C ABI ----

def test_projection_state_without_gpu(pkg):
    L, lib = pkg._lib.load(), pkg._lib
    assert (pkg.PROJ_MAX, pkg.PROJ_MIN, pkg.PROJ_MEAN) == (1, 2, 3)
    pkg.freeCudaBuffers()
    pkg.set_projection(None)
    L.vr_clear_error()
    assert pkg.projection() is None and L.vr_projection() == 0
    try:
        # set, read back, replace
        for name, value in (("max", 1), ("min", 2), ("mean", 3)):
            pkg.set_projection(name)
            assert pkg.projection() == name and L.vr_projection() == value
            pkg.set_projection(value)
            assert pkg.projection() == name
        pkg.set_projection(0)
        assert pkg.projection() is None
        with pytest.raises(ValueError):
            pkg.set_projection("median")
        # errors leave the state as it was
        pkg.set_projection("min")
        for bad in (-1, 4, 1 << 20):
            assert L.vr_set_projection(bad) == lib.VR_ERR_ARG
            assert "projection" in L.vr_last_error().decode()
            assert pkg.projection() == "min"
        L.vr_clear_error()
        # the mode is the caller's: it outlives freeCudaBuffers, the releases and the
        # other setters; nothing so far has made a device call
        pkg.freeCudaBuffers()
        pkg.release_stats()
        pkg.release_crossing()
        pkg.release_weighted()
        pkg.release_gmm_stats()
        pkg.set_bin_weights([1.0, 2.0])
        pkg.set_bin_weights(None)
        pkg.set_transfer_function(RAMP2)
        pkg.set_transfer_function(None)
        pkg.set_transfer_function_2d(np.zeros((2, 2, 4), np.float32), 1)
        pkg.set_transfer_function_2d(None)
        assert pkg.projection() == "min"
        L.vr_clear_error()
        pkg.set_projection("mean")
        assert L.vr_last_status() == lib.VR_OK and L.vr_last_error() == b""
    finally:
        pkg.set_projection(None)
        pkg.set_transfer_function(None)
        pkg.set_transfer_function_2d(None)
        L.vr_clear_error()
    assert pkg.projection() is None


def test_refusals_come_before_any_device_work(pkg):
    """with a projection set, what has no plane march is refused outright -- the counts
    before they look at their descriptor"""
    L, lib = pkg._lib.load(), pkg._lib
    pkg.freeCudaBuffers()
    d = pkg.make_desc(0x1000, W, H, camera("C0"), query_method=1, volume_size=(4, 4, 4))
    try:
        for mode, word in (("max", "maximum"), ("min", "minimum"), ("mean", "mean")):
            pkg.set_projection(mode)
            for call in (L.vr_count_footprint, L.vr_footprint_bytes, L.vr_gmm_count_footprint):
                assert call(ctypes.byref(d)) == lib.VR_ERR_UNSUPPORTED
                msg = L.vr_last_error().decode()
                assert f"{word} projection" in msg and "bake" in msg, msg
                assert "vr_set_projection(0)" in msg, msg
            assert L.vr_gmm_count_footprint_slab(ctypes.byref(d), None) == lib.VR_ERR_UNSUPPORTED
            assert L.vr_render_gmm(ctypes.byref(d), None) == lib.VR_ERR_UNSUPPORTED
            assert f"{word} projection" in L.vr_last_error().decode()
        # a 2-D table at the same time: the message says why
        pkg.set_transfer_function_2d(np.zeros((2, 2, 4), np.float32), 1)
        assert L.vr_count_footprint(ctypes.byref(d)) == lib.VR_ERR_UNSUPPORTED
        msg = L.vr_last_error().decode()
        assert "classifies one plane" in msg and "vr_set_projection(0)" in msg, msg
    finally:
        pkg.set_projection(None)
        pkg.set_transfer_function_2d(None)
        L.vr_clear_error()
    # cleared: the usual state error of a library without a volume
    assert L.vr_count_footprint(ctypes.byref(d)) == lib.VR_ERR_STATE
    L.vr_clear_error()


def test_exports(pkg):
    for name in ("PROJ_MAX", "PROJ_MIN", "PROJ_MEAN", "set_projection", "projection"):
        assert name in pkg.api.__all__ and hasattr(pkg, name), name
    for name in ("vr_set_projection", "vr_projection"):
        assert name in pkg._lib.EXPORTS and hasattr(pkg._lib.load(), name), name


# ---- the seeded sweep of tests/test_gpu_random_projection.py ----

# random_cases.tf_case's and tf_tile_case's seeds in order, each slot taking the next
# seed whose reference frame under the slot's mode has hit pixels of more than one
# colour.  The windows and tables of those cases were drawn for compositing, where a
# ray's colour depends on its length; under a projection a one-entry table (seed % 7
# == 0), an extremum that every ray of the volume attains, or a window that puts every
# ray's value beyond one end of the table makes the frame one colour, and such a frame
# compares nothing.  test_sweep_census holds the choice by the reference alone.
WHOLE_SEEDS = (2, 3, 6, 8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 19, 20, 22, 24, 25, 27, 29, 33, 34,
               36, 38, 39, 40, 41, 44, 45, 46, 47, 48, 50, 51, 52, 53, 54, 60, 61, 62)
TILE_SEEDS = (2, 6, 8, 10, 12, 16, 18, 20)  # (even: a 1-D table)
N_WHOLE, N_TILES = len(WHOLE_SEEDS), len(TILE_SEEDS)
assert (N_WHOLE, N_TILES) == (40, 8)


def proj_case(i):
    """case i of the sweep, 0 <= i < 48: random_cases' 1-D table case -- volume family,
    method (so the blend), dtype, edge shapes, view (eye inside the volume among them),
    window (negated among them), table (entries outside [0, 1] among them), knobs --
    with the mode dealt in turn; the last 8 are its multi-rank tile-list cases (the
    even seeds: a 1-D table), the modes dealt against the seeds' period of two"""
    if i < N_WHOLE:
        case = rc.tf_case(WHOLE_SEEDS[i])
    else:
        case = rc.tf_tile_case(TILE_SEEDS[i - N_WHOLE])
    assert case["v"] is None
    return dict(case, index=i, mode=MODES[(i + i // 3) % 3])


def proj_reference(case, planes, m):
    from test_random_cases import blend_of
    p = case["params"]
    return ref_projection.render_plane(planes[case["u"]], case["W"], case["H"], m, case["mode"],
                                       rc.make_table(case["table"]), blend=blend_of(case["u"]),
                                       brightness=p["brightness"], toff=p["toff"],
                                       tscale=p["tscale"])


def test_sweep_census(pkg, orc):
    """by the reference alone: every case has hit pixels of more than one colour, at
    most 4 of the 48 are degenerate (fewer than 20 hit pixels), and the sweep reaches
    what it is for"""
    from test_random_cases import camera as case_camera, eye_inside, tf_planes
    rows = []
    for i in range(N_WHOLE + N_TILES):
        case = proj_case(i)
        m = case_camera(pkg, case)
        rgba8, _, n = proj_reference(case, tf_planes(pkg, orc, case), m)
        hit = n >= 0
        rows.append(dict(case=case, hits=int(hit.sum()), colours=np.unique(rgba8[hit]).size,
                         inside=eye_inside(m), longest=int(n.max())))
    for r in rows:
        assert r["colours"] > 1, (r["case"]["index"], r["hits"], r["colours"])
    assert sum(r["hits"] < 20 for r in rows) <= 4
    count = lambda f: sum(bool(f(r)) for r in rows)
    for mode in MODES:
        for cross, least in ((False, 8), (True, 1)):  # (method 13 is one of 7 or 5 in turn)
            assert count(lambda r: r["case"]["mode"] == mode
                         and (r["case"]["u"] == 13) == cross) >= least, (mode, cross)
        assert count(lambda r: r["case"]["mode"] == mode and r["case"]["edge"]) >= 1, mode
    assert count(lambda r: r["inside"]) >= 3
    assert count(lambda r: r["case"]["negated"]) >= 3
    assert count(lambda r: r["case"]["table"]["kind"] == "wide") >= 8
    assert count(lambda r: r["case"]["knobs"].get("VR_TF_WIDE")) >= 6
    assert count(lambda r: r["case"]["family"] == "codec") >= 4
    assert count(lambda r: r["case"]["family"] == "gmm") >= 8
    assert count(lambda r: r["case"]["dtype"] == "f16") >= 8
    assert count(lambda r: r["longest"] > 4 * 20) >= 10  # rays that wrap the ring many times
