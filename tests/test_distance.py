"""The distribution-distance query (method 12) without a
GPU: the numpy statistic against answers worked by hand, the host state of the C
ABI (vr_set_query_target makes no device call), the region mean against a box
worked by hand, and the reference frames the GPU tests compare against."""
import ctypes
import functools

import numpy as np
import pytest

import __graft_entry__ as graft
import ref_distance
import ref_numpy

f32 = np.float32
BINS = (1, 2, 4, 8, 16, 32)
METRICS = ref_distance.METRICS
SMALL = (12, 10, 9)
DIMS = (24, 20, 16)
BAKE = (37, 5, 3)
W, H = 64, 48
# the target of the GPU tests' frames: the record of the volume's centre voxel
# (its distance from the synthetic volumes' records spans 0 .. 1 for L1 and KS and
# 0 .. 0.6 for EMD), at the transfer scale that puts those values on the colour table
DIST_TSCALE = 1.0
# the box of the region tests, inside the (24, 20, 16) volume: lo, hi
REGION = ((5, 3, 2), (9, 6, 4))

D = ref_distance.distance_stat


def centre_target(vol):
    """the record of the centre voxel of vol (nz, ny, nx, B), widened to float32"""
    nz, ny, nx, _ = vol.shape
    return np.asarray(vol[nz // 2, ny // 2, nx // 2]).astype(np.float32)


# ---- known answers ----

@pytest.mark.parametrize("nb", BINS)
def test_a_record_equal_to_the_target(nb):
    """every d_i is 0: D = 0 for all metrics, and the similarity is exactly 1"""
    rng = np.random.default_rng(1200 + nb)
    p = rng.random((20, nb)).astype(np.float32)
    for metric in METRICS:
        for r in p:
            got = D(r, r, metric)
            assert got.dtype == np.float32 and got == 0, (nb, metric, got)
            assert D(r, r, metric, similarity=True) == f32(1.0)


@pytest.mark.parametrize("nb", BINS[1:])
def test_point_masses(nb):
    """all mass in bin j against all mass in bin k != j: L1 = (1 + 1) / 2 = 1; the CDF
    gap is 1 on the bins from min(j, k) to max(j, k) - 1 and 0 elsewhere, so KS = 1
    and EMD = |j - k| / B exactly (small integers times a power of two)"""
    for j in range(nb):
        for k in range(nb):
            if j == k:
                continue
            p, h = np.zeros(nb, np.float32), np.zeros(nb, np.float32)
            p[j], h[k] = 1.0, 1.0
            assert D(p, h, "l1") == f32(1.0)
            assert D(p, h, "ks") == f32(1.0)
            assert D(p, h, "emd") == f32(abs(j - k)) / f32(nb)
            assert D(p, h, "emd", similarity=True) == f32(1.0) - f32(abs(j - k)) / f32(nb)


def test_power_of_two_multiples_scale_exactly():
    """every operation scales exactly by a power of two (no result is subnormal here)"""
    rng = np.random.default_rng(1207)
    p = rng.random((50, 8)).astype(np.float32)
    h = rng.random(8).astype(np.float32)
    for metric in METRICS:
        base = D(p, h, metric)
        assert np.all(base > 0)
        for s in (2.0 ** -10, 8.0):
            assert np.array_equal(D(p * f32(s), h * f32(s), metric), base * f32(s)), (metric, s)


def test_one_bin_record_by_hand():
    """B = 1, p = 0.75, h = 0.25: d = 0.5.  L1 = 0.5 * 0.5; EMD = |0.5| * (1 / 1);
    KS = max(0, 0.5)"""
    p, h = f32([0.75]), f32([0.25])
    assert D(p, h, "l1") == f32(0.25)
    assert D(p, h, "emd") == f32(0.5)
    assert D(p, h, "ks") == f32(0.5)
    assert D(p, h, "l1", similarity=True) == f32(0.75)
    # the sign of the difference does not matter
    assert D(h, p, "l1") == f32(0.25) and D(h, p, "emd") == f32(0.5) and D(h, p, "ks") == f32(0.5)


def test_unnormalised_pair_by_hand():
    """p = [2, 0, 0, 0] (total 2) against h = [0, 0, 0, 1] (total 1): d = 2 0 0 -1,
    E = 2 2 2 1.  L1 = (2 + 1) / 2.  EMD sums all four prefix differences, the last
    one being the difference of the totals: (2 + 2 + 2 + 1) / 4, where the
    Wasserstein sum over the three inner bin edges alone would give 6 / 4.
    KS = 2."""
    p, h = f32([2, 0, 0, 0]), f32([0, 0, 0, 1])
    assert np.array_equal(ref_distance.prefix(ref_distance.differences(p, h)), f32([2, 2, 2, 1]))
    assert D(p, h, "l1") == f32(1.5)
    assert D(p, h, "emd") == f32(1.75)
    assert D(p, h, "emd") != f32(1.5)
    assert D(p, h, "ks") == f32(2.0)
    assert D(p, h, "ks", similarity=True) == f32(-1.0)  # nothing is clamped


def test_a_subnormal_difference_is_kept():
    tiny = f32(1e-40)
    assert 0 < tiny < np.finfo(np.float32).tiny
    p, h = f32([1.0, 1e-40]), f32([1.0, 0.0])
    assert D(p, h, "l1") == tiny * f32(0.5) and D(p, h, "l1") > 0
    assert D(p, h, "emd") == tiny * f32(0.5)   # E = 0, 1e-40; 1 / B = 0.5
    assert D(p, h, "ks") == tiny
    # and the difference of two normal numbers that is subnormal
    a = np.finfo(np.float32).tiny
    p, h = f32([a * f32(1.5)]), f32([a])
    assert D(p, h, "ks") == a * f32(0.5) and D(p, h, "ks") > 0


def test_ks_takes_the_other_operand_for_a_nan():
    """np.fmax, as fmaxf: a NaN prefix difference is skipped, a later one counts"""
    p, h = f32([np.inf, 1.0]), f32([np.inf, 0.0])
    with np.errstate(all="ignore"):
        assert np.isnan(D(p, h, "l1")) and np.isnan(D(p, h, "emd"))
        assert D(f32([np.nan, 0.0]), f32([0.0, 0.0]), "ks") == 0
        assert D(f32([0.5, np.nan]), f32([0.0, 0.0]), "ks") == f32(0.5)


def test_region_mean_against_a_box_worked_by_hand():
    """a 4 x 3 x 2 volume of 2 bins with bin 0 = x + 10 y + 100 z and bin 1 = 0.5: the
    box [1, 3) x [0, 2) x [0, 2) holds x in {1, 2}, y in {0, 1}, z in {0, 1}, so the
    mean of bin 0 is 1.5 + 5 + 50"""
    nz, ny, nx = 2, 3, 4
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol = np.stack([x + 10 * y + 100 * z, np.full(x.shape, 0.5)], axis=-1).astype(np.float32)
    got = ref_distance.region_mean(vol, (1, 0, 0), (3, 2, 2))
    assert got.dtype == np.float32 and np.array_equal(got, f32([56.5, 0.5]))
    # one voxel: its record; an f16 volume is widened first
    assert np.array_equal(ref_distance.region_mean(vol, (3, 2, 1), (4, 3, 2)), f32([123, 0.5]))
    third = np.full((1, 1, 3, 1), 1.0 / 3.0, np.float16)
    want = f32(3.0 * float(np.float16(1.0 / 3.0)) / 3.0)
    assert np.array_equal(ref_distance.region_mean(third, (0, 0, 0), (3, 1, 1)), [want])
    # the sum is taken in double and rounded once: 2^24 + 1 + 1 + 1 keeps its ones
    big = np.array([2.0 ** 24, 1.0, 1.0, 1.0], np.float32).reshape(1, 1, 4, 1)
    assert ref_distance.region_mean(big, (0, 0, 0), (4, 1, 1))[0] == f32((2.0 ** 24 + 3.0) / 4.0)


# ---- host state of the C ABI ----

def test_target_state_without_gpu(pkg):
    L = pkg._lib.load()
    lib = pkg._lib
    pkg.freeCudaBuffers()
    pkg.set_query_target(None)
    with pytest.raises(pkg.VRError) as e:
        pkg.query_target()
    assert e.value.status == lib.VR_ERR_STATE
    # set, read back, replace, clear
    for nb in BINS:
        h = (np.arange(nb, dtype=np.float32) + f32(0.25)) / f32(nb)
        for metric in METRICS:
            for sim in (False, True):
                pkg.set_query_target(h, metric, sim)
                got = pkg.query_target()
                assert np.array_equal(got[0], h) and got[0].dtype == np.float32
                assert got[1:] == (metric, sim)
    # integer metrics, and a similarity flag that is any non-zero int
    a = f32([0.5, 0.25])
    assert L.vr_set_query_target(a.ctypes.data, 2, lib.VR_DIST_KS, 7) == lib.VR_OK
    assert pkg.query_target()[1:] == ("ks", True)
    assert (lib.VR_DIST_L1, lib.VR_DIST_EMD, lib.VR_DIST_KS) == (0, 1, 2)
    # NULL arguments
    n, mt = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.vr_query_target(None, ctypes.addressof(n), None, None) == lib.VR_OK and n.value == 2
    assert L.vr_query_target(None, None, ctypes.addressof(mt), None) == lib.VR_OK and mt.value == 2
    assert L.vr_query_target(None, None, None, None) == lib.VR_OK
    # errors leave the state as it was
    keep = f32([0.125, 0.5, 0.25, 0.125])
    pkg.set_query_target(keep, "emd", True)

    def unchanged():
        got = pkg.query_target()
        return np.array_equal(got[0], keep) and got[1:] == ("emd", True)

    for n_bad in (0, 3, 5, 6, 12, 33, 64, -1):
        b = np.zeros(max(n_bad, 1), np.float32)
        assert L.vr_set_query_target(b.ctypes.data, n_bad, 0, 0) == lib.VR_ERR_UNSUPPORTED
        assert unchanged()
    for bad in (float("nan"), float("inf"), float("-inf")):
        b = f32([0.5, bad])
        assert L.vr_set_query_target(b.ctypes.data, 2, 0, 0) == lib.VR_ERR_ARG
        assert unchanged()
    for m_bad in (-1, 3, 12):
        assert L.vr_set_query_target(a.ctypes.data, 2, m_bad, 0) == lib.VR_ERR_ARG
        assert unchanged()
    with pytest.raises(ValueError):
        pkg.set_query_target(a, "cosine")
    # the region setter needs a record volume
    assert L.vr_set_query_target_region(0, 0, 0, 1, 1, 1, 0, 0) == lib.VR_ERR_STATE
    with pytest.raises(pkg.VRError) as e:
        pkg.set_query_target_region((0, 0, 0), (1, 1, 1))
    assert e.value.status == lib.VR_ERR_STATE
    assert unchanged()
    # no plane, and nothing to bake, without a volume
    assert pkg.distance_info() == (None, 0)
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_distance()
    assert e.value.status == lib.VR_ERR_STATE
    pkg.release_distance()
    assert unchanged()  # releasing the plane keeps the target
    pkg.set_query_target(None)
    with pytest.raises(pkg.VRError) as e:
        pkg.query_target()
    assert e.value.status == lib.VR_ERR_STATE
    with pytest.raises(pkg.VRError) as e:  # nothing set and no volume
        pkg.bake_distance()
    assert e.value.status == lib.VR_ERR_STATE
    L.vr_clear_error()


def test_target_state_is_apart_from_weights_and_quantile(pkg):
    pkg.set_bin_weights([1.0, 2.0])
    pkg.set_quantile(0.5)
    pkg.set_query_target([0.5, 0.5], "ks")
    pkg.set_bin_weights(None)
    pkg.set_quantile(None)
    got = pkg.query_target()
    assert np.array_equal(got[0], f32([0.5, 0.5])) and got[1:] == ("ks", False)
    pkg.set_bin_weights([1.0, 2.0])
    pkg.set_quantile(0.25)
    pkg.set_query_target(None)
    assert np.array_equal(pkg.bin_weights(), f32([1.0, 2.0]))
    assert pkg.quantile() == (0.25, 0.25, False)
    pkg.set_bin_weights(None)
    pkg.set_quantile(None)


def test_render_method_12_without_volume(pkg):
    L = pkg._lib.load()
    pkg.freeCudaBuffers()
    pkg.set_query_target([0.5, 0.5])
    d = pkg.make_desc(0x1000, W, H, pkg.camera.single_test_inv_view(),
                      query_method=pkg.QUERY_DISTANCE, volume_size=(4, 4, 4))
    assert pkg.QUERY_DISTANCE == 12
    assert L.vr_render(ctypes.byref(d)) == pkg._lib.VR_ERR_STATE
    with pytest.raises(pkg.VRError) as e:
        pkg.render_kernel((4, 12, 1), (16, 4, 1), 0x1000, W, H, 0.05, 1.0, 0.0, 1.0, 12, (4, 4, 4))
    assert e.value.status == pkg._lib.VR_ERR_STATE
    assert L.vr_count_footprint(ctypes.byref(d)) == pkg._lib.VR_ERR_UNSUPPORTED
    assert L.vr_footprint_bytes(ctypes.byref(d)) == pkg._lib.VR_ERR_UNSUPPORTED
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_distance()
    assert e.value.status == pkg._lib.VR_ERR_STATE
    L.vr_clear_error()
    pkg.set_query_target(None)


def test_exports(pkg):
    for name in ("QUERY_DISTANCE", "set_query_target", "query_target", "set_query_target_region",
                 "bake_distance", "release_distance", "distance_info"):
        assert name in pkg.api.__all__ and hasattr(pkg, name), name


# ---- the numpy reference ----

@functools.lru_cache(maxsize=None)
def _volume(orc_synth, dims, nb):
    v = orc_synth(*dims, nb)
    v.setflags(write=False)
    return v


def camera(cam):
    pkg = graft.load_package()
    if cam == "C0":
        return pkg.camera.single_test_inv_view()
    return pkg.camera.display_inv_view((0.0, 90.0) if cam == "S" else (30.0, 45.0))


@functools.lru_cache(maxsize=None)
def volume(dims, nb, dtype):
    """the synthetic records of the tests, "f32" or narrowed to "f16"; read-only"""
    v = _volume(graft.load_oracle().synth_volume, dims, nb)
    if dtype == "f16":
        v = v.astype(np.float16)
        v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def target(dims, nb, dtype, kind="centre"):
    """the targets of the frames: the centre voxel's record, or the mean of REGION"""
    v = volume(dims, nb, dtype)
    h = centre_target(v) if kind == "centre" else ref_distance.region_mean(v, *REGION)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def reference(dims, nb, dtype, metric, sim, cam, w, h, kind="centre"):
    """the numpy frame, computed once per case and shared by the CPU and the GPU
    tests: (RGBA8, float RGBA, samples), read-only"""
    ref = ref_distance.render(volume(dims, nb, dtype), target(dims, nb, dtype, kind), metric, sim,
                              w, h, camera(cam), tscale=DIST_TSCALE)
    for a in ref:
        a.setflags(write=False)
    return ref


def test_reference_statistic_is_what_the_frame_samples(orc):
    vol = _volume(orc.synth_volume, DIMS, 8)
    h = centre_target(vol)
    p64, h64 = vol.astype(np.float64), h.astype(np.float64)
    cdf = np.cumsum(p64 - h64, axis=-1)
    for metric, want in (("l1", 0.5 * np.abs(p64 - h64).sum(-1)),
                         ("emd", np.abs(cdf).sum(-1) / 8.0), ("ks", np.abs(cdf).max(-1))):
        s = D(vol, h, metric)
        assert s.dtype == np.float32 and s.shape == vol.shape[:-1]
        assert np.unique(s).size > 100
        assert np.max(np.abs(s - want)) < 1e-5  # the textbook formula, in double
        assert np.array_equal(D(vol, h, metric, similarity=True), f32(1.0) - s)
        saved = ref_numpy.stat
        with ref_distance.distance_as_stat(h, metric, False):
            assert np.array_equal(ref_numpy.stat(vol, 0), s)
        assert ref_numpy.stat is saved
    nz, ny, nx, _ = vol.shape
    assert D(vol, h, "l1")[nz // 2, ny // 2, nx // 2] == 0


def _hits_and_colours(rgba8, n):
    hit = n >= 0
    return int(hit.sum()), int(np.unique(rgba8[hit] & 0x00FFFFFF).size) if hit.any() else 0


# the frames the GPU tests compare against: (dims, nb, dtype, metric, similarity,
# view, width, height, target kind)
GPU_FRAMES = (
    [(SMALL, nb, dt, mt, False, "C0", W, H, "centre")
     for nb in BINS for dt in ("f32", "f16") for mt in METRICS]
    + [(DIMS, 8, dt, mt, sim, "C0", W, H, "centre")
       for dt in ("f32", "f16") for mt in METRICS for sim in (False, True)]
    + [(DIMS, 8, dt, "emd", False, cam, w, h, "centre")
       for dt in ("f32", "f16") for cam, w, h in (("C1", W, H), ("S", W, H), ("C1", 70, 50))]
    + [(DIMS, 8, dt, "l1", True, "C0", W, H, "region") for dt in ("f32", "f16")]
    + [(BAKE, 4, dt, "ks", False, cam, W, H, "centre")
       for dt in ("f32", "f16") for cam in ("C0", "C1", "S")]
)


@pytest.mark.parametrize("case", GPU_FRAMES, ids=lambda c: "-".join(
    "x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c))
def test_reference_frame_has_hits_and_colours(case):
    """every reference frame of the GPU tests has hit pixels and more than one
    distinct colour among them, by the reference alone"""
    rgba8, _, n = reference(*case)
    hits, colours = _hits_and_colours(rgba8, n)
    print(f"{hits} hit, {colours} colours")
    assert hits > 20 and colours > 1, (case, hits, colours)
