"""The weighted-bin query (method 10) without a GPU: the
range weights, the host state of the C ABI (vr_set_bin_weights and friends make
no device call) and the numpy reference the GPU tests compare against."""
import ctypes
import functools

import numpy as np
import pytest

import ref_numpy
import ref_weighted

f32 = np.float32
BINS = (1, 2, 4, 8, 16, 32)
DIMS = (24, 20, 16)
W, H = 64, 48


def test_range_weights_known_answers(pkg):
    rw = pkg.range_weights
    for n in BINS:
        w = rw(0.0, 1.0, n)
        assert w.dtype == np.float32 and w.shape == (n,)
        assert np.array_equal(w, np.ones(n, np.float32))
    assert np.array_equal(rw(0.25, 0.75, 8), f32([0, 0, 1, 1, 1, 1, 0, 0]))
    # a bound inside a bin: [0.3, 0.3125) lies in bin 4 of 16, [0.25, 0.3125).  The
    # bounds are float32: 0.3f = 0.300000011920928955078125, so the covered part is
    # 0.3125 - 0.3f = 0.012499988079071044921875 and 16 times that, a float32,
    # is 0.19999980926513671875
    w = rw(0.3, 0.3125, 16)
    want = np.zeros(16, np.float32)
    want[4] = f32(0.19999980926513671875)
    assert float(want[4]) == 16.0 * (0.3125 - float(f32(0.3)))
    assert np.array_equal(w, want), w
    # both bounds inside bins: [0.3, 0.7) of 4 bins covers 0.8 of bin 1 and of bin 2
    w = rw(0.3, 0.7, 4)
    assert np.array_equal(w, f32([0.0, 4.0 * (0.5 - float(f32(0.3))),
                                  4.0 * (float(f32(0.7)) - 0.5), 0.0])), w
    # an empty range and a range outside [0, 1)
    assert not rw(0.4, 0.4, 8).any() and not rw(1.5, 2.0, 8).any()
    assert np.array_equal(rw(-1.0, 2.0, 8), np.ones(8, np.float32))


@pytest.mark.parametrize("n", BINS)
def test_range_weights_sum(pkg, n):
    """the weights sum to n (hi - lo) within 1 ulp (of 1.0f) per covered bin"""
    rng = np.random.default_rng(410 + n)
    for _ in range(50):
        lo, hi = np.sort(rng.random(2).astype(np.float32))
        w = pkg.range_weights(lo, hi, n)
        assert np.all(w >= 0) and np.all(w <= 1)
        covered = int(np.count_nonzero(w))
        assert abs(float(np.sum(w.astype(np.float64))) - n * (float(hi) - float(lo))) \
            <= covered * 2.0 ** -23


def test_range_weights_needs_no_library(pkg):
    """a pure function: it validates its arguments itself"""
    with pytest.raises(ValueError):
        pkg.range_weights(0.5, 0.25, 8)
    with pytest.raises(ValueError):
        pkg.range_weights(0.0, float("nan"), 8)
    with pytest.raises(ValueError):
        pkg.range_weights(0.0, 1.0, 0)
    assert pkg.range_weights(0.0, 0.5, 6).shape == (6,)  # any n: only the library limits it


def test_query_range_equals_range_weights(pkg):
    """vr_set_query_range then vr_bin_weights == range_weights, bit for bit, for the
    supported n of 1 .. 32; every other n is VR_ERR_UNSUPPORTED"""
    L = pkg._lib.load()
    rng = np.random.default_rng(20261019)
    bounds = [(0.0, 1.0), (0.25, 0.75), (0.2, 0.7), (0.3, 0.3125), (0.4, 0.4), (-0.5, 0.1),
              (0.9, 3.0)]
    bounds += [tuple(np.sort(rng.random(2))) for _ in range(20)]
    for n in range(1, 33):
        for lo, hi in bounds:
            st = L.vr_set_query_range(lo, hi, n)
            if n not in BINS:
                assert st == pkg._lib.VR_ERR_UNSUPPORTED
                continue
            assert st == pkg._lib.VR_OK
            got = pkg.bin_weights()
            want = pkg.range_weights(lo, hi, n)
            assert got.shape == (n,)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, lo, hi)
    L.vr_clear_error()
    pkg.set_bin_weights(None)


def test_weight_state_without_gpu(pkg):
    L = pkg._lib.load()
    lib = pkg._lib
    pkg.freeCudaBuffers()
    pkg.set_bin_weights(None)
    with pytest.raises(pkg.VRError) as e:
        pkg.bin_weights()
    assert e.value.status == lib.VR_ERR_STATE
    # set, read back, replace, clear
    w = f32([0.5, -2.0, 0.0, 1e-39, 3.0, -0.0, 7.25, 1e30])
    pkg.set_bin_weights(w)
    assert np.array_equal(pkg.bin_weights().view(np.uint32), w.view(np.uint32))
    pkg.set_bin_weights([1.0, 2.0])
    assert np.array_equal(pkg.bin_weights(), f32([1.0, 2.0]))
    n = ctypes.c_int(-1)
    assert L.vr_bin_weights(None, ctypes.addressof(n)) == lib.VR_OK and n.value == 2
    # counts outside 1, 2, 4, 8, 16, 32
    for bad in (0, 3, 6, 33, 64, -1):
        buf = np.ones(64, np.float32)
        assert L.vr_set_bin_weights(buf.ctypes.data, bad) == lib.VR_ERR_UNSUPPORTED
    # non-finite weights
    for v in (np.inf, -np.inf, np.nan):
        buf = np.ones(8, np.float32)
        buf[5] = v
        assert L.vr_set_bin_weights(buf.ctypes.data, 8) == lib.VR_ERR_ARG
    # a refused call leaves the weights as they were
    assert np.array_equal(pkg.bin_weights(), f32([1.0, 2.0]))
    # range bounds
    assert L.vr_set_query_range(0.75, 0.25, 8) == lib.VR_ERR_ARG
    assert L.vr_set_query_range(float("nan"), 0.25, 8) == lib.VR_ERR_ARG
    assert L.vr_set_query_range(0.0, float("inf"), 8) == lib.VR_ERR_ARG
    assert L.vr_set_query_range(0.0, 1.0, 5) == lib.VR_ERR_UNSUPPORTED
    # no plane, and nothing to bake, without a volume
    assert pkg.weighted_info() == (None, 0)
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_weighted()
    assert e.value.status == lib.VR_ERR_STATE
    pkg.release_weighted()
    pkg.set_bin_weights(None)
    with pytest.raises(pkg.VRError) as e:
        pkg.bin_weights()
    assert e.value.status == lib.VR_ERR_STATE
    L.vr_clear_error()


def test_render_method_10_without_volume(pkg):
    L = pkg._lib.load()
    pkg.freeCudaBuffers()
    pkg.set_query_range(0.25, 0.75, 8)
    d = pkg.make_desc(0x1000, W, H, pkg.camera.single_test_inv_view(),
                      query_method=pkg.QUERY_WEIGHTED, volume_size=(4, 4, 4))
    assert pkg.QUERY_WEIGHTED == 10
    assert L.vr_render(ctypes.byref(d)) == pkg._lib.VR_ERR_STATE
    with pytest.raises(pkg.VRError) as e:
        pkg.render_kernel((4, 12, 1), (16, 4, 1), 0x1000, W, H, 0.05, 1.0, 0.0, 1.0, 10, (4, 4, 4))
    assert e.value.status == pkg._lib.VR_ERR_STATE
    assert L.vr_count_footprint(ctypes.byref(d)) == pkg._lib.VR_ERR_UNSUPPORTED
    assert L.vr_footprint_bytes(ctypes.byref(d)) == pkg._lib.VR_ERR_UNSUPPORTED
    L.vr_clear_error()
    pkg.set_bin_weights(None)


# ---- the numpy reference ----

@functools.lru_cache(maxsize=None)
def _volume(orc_synth):
    v = orc_synth(*DIMS, 8)
    v.setflags(write=False)
    return v


def test_reference_all_ones_is_the_record_sum(orc):
    vol = _volume(orc.synth_volume)
    s = ref_weighted.lin_stat(vol, np.ones(8, np.float32))
    want = np.zeros(vol.shape[:-1], np.float32)
    for i in range(8):  # the float32 sum of the bins in order, 0 + p_0 first
        want = want + vol[..., i]
    assert s.dtype == np.float32 and np.array_equal(s, want)
    assert np.all(np.abs(s - 1) < 1e-5)  # the synthetic records are normalised histograms
    # and the patched statistic is what ref_numpy.render samples, then restored
    saved = ref_numpy.stat
    with ref_weighted.weighted_stat(np.ones(8, np.float32)):
        assert np.array_equal(ref_numpy.stat(vol, 0), want)
    assert ref_numpy.stat is saved


def test_reference_subnormal_products_are_kept():
    p = f32([[0.5, 0.25, 0.125, 0.0625]])
    w = (f32(1e-39) * np.arange(1, 5, dtype=np.float32)).astype(np.float32)
    s = ref_weighted.lin_stat(p, w)
    assert s[0] != 0 and abs(float(s[0])) < float(np.finfo(np.float32).tiny)
    acc = f32(0)
    for i in range(4):
        acc = f32(acc + f32(p[0, i] * w[i]))
    assert s[0] == acc


def test_reference_frame_takes_both_exits(pkg, orc):
    """the frame the GPU tests compare against (24 x 20 x 16 x 8, C0, 64 x 48, the
    seeded weights of both signs) has rays that stop on opacity > 0.95 and rays
    that leave the box: against the same frame at density 0, where no ray can turn
    opaque, the first take fewer samples and the second exactly as many"""
    vol = _volume(orc.synth_volume)
    w = ref_weighted.seeded_weights(8)
    assert (w > 0).any() and (w < 0).any()
    m = pkg.camera.single_test_inv_view()
    _, rgba, n = ref_weighted.render(vol, w, W, H, m)
    _, _, n_box = ref_weighted.render(vol, w, W, H, m, density=0.0)
    hit = n_box >= 0
    assert np.array_equal(n >= 0, hit) and hit.any() and (~hit).any()
    assert np.all(n[hit] <= n_box[hit]) and np.all(n_box[hit] < 500)
    early = hit & (n < n_box)
    through = hit & (n == n_box) & (rgba[..., 3] <= 0.95)
    print(f"rays: {int(hit.sum())} hit, {int(early.sum())} end on opacity, "
          f"{int(through.sum())} leave the box")
    assert early.sum() >= 1 and through.sum() >= 1
    assert np.all(rgba[early][:, 3] > 0.95)
