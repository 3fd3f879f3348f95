"""The quantile query (method 11) without a GPU: the numpy
statistic against answers worked by hand, the host state of the C ABI
(vr_set_quantile and friends make no device call) and the reference frames the
GPU tests compare against."""
import ctypes
import functools

import numpy as np
import pytest

import ref_numpy
import ref_quantile

f32 = np.float32
BINS = (1, 2, 4, 8, 16, 32)
DIMS = (24, 20, 16)
W, H = 64, 48
# the spread frame of the GPU tests: the interquartile range, and the transfer
# scale that spreads its values (0.06 .. 0.17 here) over more of the colour table
SPREAD = (0.25, 0.75)
SPREAD_TSCALE = 2.5

Q = ref_quantile.quantile_stat


# ---- known answers ----

@pytest.mark.parametrize("nb", BINS)
def test_uniform_record_is_the_identity(nb):
    """p_i = 1 / B: every c_i, tau - c_{k-1} and the division by 1 / B are exact and
    k + frac = q B is a float, so Q(q) == q bit for bit"""
    p = np.full(nb, f32(1.0 / nb), np.float32)
    rng = np.random.default_rng(1100 + nb)
    qs = np.concatenate([f32([0.0, 1.0, 0.5, 0.25, 1.0 / nb]), rng.random(200).astype(np.float32)])
    for q in qs:
        got = Q(p, float(q))
        assert got.dtype == np.float32 and got == q, (nb, q, got)


def test_all_mass_in_one_bin():
    """mass 2 in bin j of 8: tau = 2 q, frac = 2 q / 2 = q exactly, Q = (j + q) / 8"""
    for j in range(8):
        p = np.zeros(8, np.float32)
        p[j] = 2.0
        for q in (0.0, 0.125, 0.5, 0.7, 1.0):
            want = f32(f32(j) + f32(q)) * f32(0.125)
            assert Q(p, q) == want, (j, q)
    # first, middle and last bin at the median: the bin's centre
    for j, want in ((0, 0.0625), (3, 0.4375), (7, 0.9375)):
        p = np.zeros(8, np.float32)
        p[j] = 2.0
        assert Q(p, 0.5) == f32(want)


def test_a_tie_takes_the_lower_bin():
    """p = [0.5, 0.5], q = 0.5: c_0 = tau, so k = 0 and frac = (0.5 - 0) / 0.5 = 1:
    the edge between the bins, reached from below"""
    assert Q(f32([0.5, 0.5]), 0.5) == f32(0.5)
    # the same tie with an empty bin between: still k = 0, not the empty bin
    assert Q(f32([0.5, 0.0, 0.5, 0.0]), 0.5) == f32(0.25)
    # just above the tie the quantile jumps over the empty bin
    q = float(np.nextafter(f32(0.5), f32(1)))
    got = Q(f32([0.5, 0.0, 0.5, 0.0]), q)
    assert f32(0.5) <= got < f32(0.5001)


def test_empty_bins_at_the_ends():
    """Q(0) is the lower edge of the support, Q(1) the upper edge"""
    p = f32([0, 0, 1, 2, 1, 0, 0, 0])
    # c = 0 0 1 3 4 4 4 4.  q = 0: tau = 0, the first i with p_i > 0 is 2, frac = 0.
    assert Q(p, 0.0) == f32(0.25)
    # q = 1: tau = 4 = c_4 (bins 5 .. 7 also reach it but are empty), frac = (4 - 3) / 1
    assert Q(p, 1.0) == f32(0.625)
    assert Q(p, 0.5) == f32(0.4375)  # tau = 2 in bin 3: (3 + (2 - 1) / 2) / 8
    assert Q(p, SPREAD) == f32(f32(0.5) - f32(0.375))


def test_empty_record_is_zero():
    for nb in BINS:
        for q in (0.0, 0.5, 1.0, (0.25, 0.75)):
            assert Q(np.zeros(nb, np.float32), q) == 0
    # as is a record whose total is not positive
    assert Q(f32([1.0, -1.0]), 0.5) == 0
    assert Q(f32([-1.0, 0.5]), 0.5) == 0


def test_unnormalised_totals():
    """no normalisation: a power-of-two multiple of a record has the same quantiles
    bit for bit (every operation scales exactly), any other multiple nearly"""
    rng = np.random.default_rng(1107)
    p = rng.random((50, 8)).astype(np.float32)
    for q in (0.0, 0.1, 0.5, 0.9, 1.0, SPREAD):
        base = Q(p, q)
        assert np.all((base >= 0) & (base <= 1))
        for s in (2.0 ** -10, 8.0):
            assert np.array_equal(Q(p * f32(s), q), base)
        for s in (1e-3, 3.7):
            assert np.max(np.abs(Q(p * f32(s), q) - base)) < 1e-6
    # worked by hand, total 4: tau = 0.75 * 4 = 3 = c_2 -> k = 2, frac = (3 - 2) / 1
    assert Q(f32([1, 1, 1, 1]), 0.75) == f32(0.75)


def test_spread_of_a_one_bin_record():
    """(q_hi - q_lo) / B: one float subtraction of the two quantiles"""
    assert Q(f32([4.0]), (0.25, 0.75)) == f32(0.5)
    assert Q(f32([4.0]), (0.3, 0.3)) == 0
    lo, hi = f32(0.3), f32(0.9)
    assert Q(f32([4.0]), (0.3, 0.9)) == hi - lo
    for j in range(8):
        p = np.zeros(8, np.float32)
        p[j] = 0.5
        assert Q(p, (0.25, 0.75)) == f32(0.0625)
        assert Q(p, (0.0, 1.0)) == f32(0.125)


def test_negative_bins_and_subnormal_quotients_follow_the_formula():
    # c = 1, 0.5, 1.5; T = 1.5; tau = 0.75: k = 0 (c_0 = 1 >= 0.75), frac = 0.75
    assert Q(f32([1.0, -0.5, 1.0, 0.0]), 0.5) == f32(0.1875)
    # a subnormal quotient is kept: tau - c_{k-1} = 1e-40 q over p_k = 1
    tiny = f32(1e-40)
    assert 0 < tiny < np.finfo(np.float32).tiny
    p = f32([1e-40, 1.0])
    # tau = 0.5 * (1e-40 + 1) = 0.5; k = 1; frac = (0.5 - 1e-40) / 1 = 0.5
    assert Q(p, 0.5) == f32(0.75)
    # q = 0 on a record starting with a subnormal bin: k = 0, frac = 0 / 1e-40 = 0
    assert Q(p, 0.0) == 0
    # frac itself subnormal: q = 1e-40 on [1, 1] gives tau = 2e-40, frac = 2e-40 / 1
    # and Q = 2e-40 / 2
    got = Q(f32([1.0, 1.0]), float(tiny))
    assert got == tiny


# ---- host state of the C ABI ----

def test_quantile_state_without_gpu(pkg):
    L = pkg._lib.load()
    lib = pkg._lib
    pkg.freeCudaBuffers()
    pkg.set_quantile(None)
    with pytest.raises(pkg.VRError) as e:
        pkg.quantile()
    assert e.value.status == lib.VR_ERR_STATE
    # set, read back, replace, clear
    pkg.set_quantile(0.3)
    assert pkg.quantile() == (float(f32(0.3)), float(f32(0.3)), False)
    pkg.set_quantile_spread(0.25, 0.75)
    assert pkg.quantile() == (0.25, 0.75, True)
    pkg.set_quantile_spread(0.5, 0.5)  # an empty spread is a spread
    assert pkg.quantile() == (0.5, 0.5, True)
    for q in (0.0, 1.0):
        pkg.set_quantile(q)
        assert pkg.quantile() == (q, q, False)
    # NULL arguments
    sp = ctypes.c_int(-1)
    assert L.vr_quantile(None, None, ctypes.addressof(sp)) == lib.VR_OK and sp.value == 0
    assert L.vr_quantile(None, None, None) == lib.VR_OK
    # bad values: refused, and the state stays as it was
    pkg.set_quantile_spread(0.125, 0.875)
    for bad in (-0.001, 1.001, float("nan"), float("inf"), float("-inf")):
        assert L.vr_set_quantile(bad) == lib.VR_ERR_ARG
        assert L.vr_set_quantile_spread(bad, 1.0) == lib.VR_ERR_ARG
        assert L.vr_set_quantile_spread(0.0, bad) == lib.VR_ERR_ARG
    assert L.vr_set_quantile_spread(0.75, 0.25) == lib.VR_ERR_ARG
    assert pkg.quantile() == (0.125, 0.875, True)
    # no plane, and nothing to bake, without a volume
    assert pkg.quantile_info() == (None, 0)
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_quantile()
    assert e.value.status == lib.VR_ERR_STATE
    pkg.release_quantile()
    assert pkg.quantile() == (0.125, 0.875, True)  # releasing the plane keeps the quantile
    pkg.set_quantile(None)
    with pytest.raises(pkg.VRError) as e:
        pkg.quantile()
    assert e.value.status == lib.VR_ERR_STATE
    with pytest.raises(pkg.VRError) as e:  # nothing set and no volume
        pkg.bake_quantile()
    assert e.value.status == lib.VR_ERR_STATE
    L.vr_clear_error()


def test_quantile_state_is_apart_from_the_bin_weights(pkg):
    pkg.set_bin_weights([1.0, 2.0])
    pkg.set_quantile(0.5)
    pkg.set_bin_weights(None)
    assert pkg.quantile() == (0.5, 0.5, False)
    pkg.set_bin_weights([1.0, 2.0])
    pkg.set_quantile(None)
    assert np.array_equal(pkg.bin_weights(), f32([1.0, 2.0]))
    pkg.set_bin_weights(None)


def test_render_method_11_without_volume(pkg):
    L = pkg._lib.load()
    pkg.freeCudaBuffers()
    pkg.set_quantile(0.5)
    d = pkg.make_desc(0x1000, W, H, pkg.camera.single_test_inv_view(),
                      query_method=pkg.QUERY_QUANTILE, volume_size=(4, 4, 4))
    assert pkg.QUERY_QUANTILE == 11
    assert L.vr_render(ctypes.byref(d)) == pkg._lib.VR_ERR_STATE
    with pytest.raises(pkg.VRError) as e:
        pkg.render_kernel((4, 12, 1), (16, 4, 1), 0x1000, W, H, 0.05, 1.0, 0.0, 1.0, 11, (4, 4, 4))
    assert e.value.status == pkg._lib.VR_ERR_STATE
    assert L.vr_count_footprint(ctypes.byref(d)) == pkg._lib.VR_ERR_UNSUPPORTED
    assert L.vr_footprint_bytes(ctypes.byref(d)) == pkg._lib.VR_ERR_UNSUPPORTED
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_quantile()
    assert e.value.status == pkg._lib.VR_ERR_STATE
    L.vr_clear_error()
    pkg.set_quantile(None)


def test_exports(pkg):
    for name in ("QUERY_QUANTILE", "set_quantile", "set_quantile_spread", "quantile",
                 "bake_quantile", "release_quantile", "quantile_info"):
        assert name in pkg.api.__all__ and hasattr(pkg, name), name


# ---- the numpy reference ----

@functools.lru_cache(maxsize=None)
def _volume(orc_synth):
    v = orc_synth(*DIMS, 8)
    v.setflags(write=False)
    return v


def test_reference_statistic_is_what_the_frame_samples(orc):
    vol = _volume(orc.synth_volume)
    s = Q(vol, 0.5)
    assert s.dtype == np.float32 and s.shape == vol.shape[:-1]
    assert np.all((s >= 0) & (s <= 1)) and np.unique(s).size > 100
    # the median lies where the CDF of the normalised record reaches one half
    cdf = np.cumsum(vol.astype(np.float64), axis=-1)
    cdf /= cdf[..., -1:]
    k = np.minimum((s.astype(np.float64) * 8).astype(int), 7)
    lo = np.where(k > 0, np.take_along_axis(cdf, np.maximum(k - 1, 0)[..., None], -1)[..., 0], 0.0)
    hi = np.take_along_axis(cdf, k[..., None], -1)[..., 0]
    assert np.all((lo <= 0.5 + 1e-6) & (hi >= 0.5 - 1e-6))
    # monotone in q, and the spread is the difference of its two quantiles
    q25, q75 = Q(vol, 0.25), Q(vol, 0.75)
    assert np.all(q25 <= s) and np.all(s <= q75)
    assert np.array_equal(Q(vol, SPREAD), q75 - q25)
    saved = ref_numpy.stat
    with ref_quantile.quantile_as_stat(0.5):
        assert np.array_equal(ref_numpy.stat(vol, 0), s)
    assert ref_numpy.stat is saved


def _exits(pkg, vol, q, m, **kw):
    """(frame RGBA8, rays that end on opacity, rays that leave the box): against the
    same frame at density 0, where no ray can turn opaque, the first take fewer
    samples and the second exactly as many"""
    rgba8, rgba, n = ref_quantile.render(vol, q, W, H, m, **kw)
    _, _, n_box = ref_quantile.render(vol, q, W, H, m, density=0.0, **kw)
    hit = n_box >= 0
    assert np.array_equal(n >= 0, hit) and hit.any() and (~hit).any()
    assert np.all(n[hit] <= n_box[hit]) and np.all(n_box[hit] < 500)
    early = hit & (n < n_box)
    through = hit & (n == n_box) & (rgba[..., 3] <= 0.95)
    assert np.all(rgba[early][:, 3] > 0.95)
    return rgba8, hit, int(early.sum()), int(through.sum())


@pytest.mark.parametrize("cam,q,want", [("C0", 0.5, (527, 861)), ("C1", 0.5, (574, 756)),
                                        ("C0", 0.9, None)])
def test_reference_frame_takes_both_exits(pkg, orc, cam, q, want):
    """the frames the GPU tests compare against (24 x 20 x 16 x 8, 64 x 48) have
    rays that stop on opacity > 0.95 and rays that leave the box; at the median
    527 and 861 of them at C0, 574 and 756 at C1"""
    vol = _volume(orc.synth_volume)
    m = (pkg.camera.single_test_inv_view() if cam == "C0"
         else pkg.camera.display_inv_view((30.0, 45.0)))
    _, hit, early, through = _exits(pkg, vol, q, m)
    print(f"{cam} q={q}: {int(hit.sum())} hit, {early} end on opacity, {through} leave the box")
    assert early >= 1 and through >= 1
    if want:
        assert (early, through) == want


def test_reference_spread_frame_has_hits_and_colours(pkg, orc):
    """the spread frame of the GPU tests, (0.25, 0.75) at transfer scale 2.5"""
    vol = _volume(orc.synth_volume)
    m = pkg.camera.single_test_inv_view()
    s = Q(vol, SPREAD)
    print(f"spread of the volume: {s.min():.4f} .. {s.max():.4f}")
    assert s.min() >= 0 and s.max() * SPREAD_TSCALE <= 1.0 and np.unique(s).size > 100
    rgba8, hit, early, through = _exits(pkg, vol, SPREAD, m, tscale=SPREAD_TSCALE)
    colours = np.unique(rgba8[hit] & 0x00FFFFFF)
    print(f"spread: {int(hit.sum())} hit, {early} end on opacity, {through} leave the box, "
          f"{colours.size} colours")
    assert hit.sum() > 100 and colours.size > 1
