"""The level-crossing query (method 13) without a GPU: the
numpy combine against answers worked by hand, the restated march loop against
ref_weighted's frames, the host state of the C ABI (vr_set_crossing_weights and
vr_set_isovalue make no device call), and the reference frames the GPU tests
compare against."""
import ctypes
import functools

import numpy as np
import pytest

import __graft_entry__ as graft
import ref_crossing
import ref_weighted

f32 = np.float32
BINS = (1, 2, 4, 8, 16, 32)
SMALL = (12, 10, 9)
DIMS = (24, 20, 16)
BAKE = (37, 5, 3)
W, H = 64, 48
THETA = 0.3  # the isovalue of every reference frame

C = ref_crossing.combine


def F8(*v):
    assert len(v) == 8
    return np.array(v, dtype=np.float32)


# ---- known answers of the combine ----

def test_known_answers():
    """lo = prod F_c, hi = prod (1 - F_c), s = (1 - lo) - hi"""
    cases = (
        (F8(0, 0, 0, 0, 0, 0, 0, 0), 0.0),          # lo 0, hi 1: surely all above
        (F8(1, 1, 1, 1, 1, 1, 1, 1), 0.0),          # lo 1, hi 0: surely all below
        (F8(0, 1, 0, 1, 1, 0, 1, 0), 1.0),          # both products hold a 0
        (F8(0, 0, 0, 1, 0, 0, 0, 0), 1.0),
        (F8(*[0.5] * 8), 0.9921875),                # 1 - 2^-8 - 2^-8, every step exact
        (F8(0.5, 1, 1, 1, 1, 1, 1, 1), 0.5),        # lo 0.5, hi 0
    )
    for F, want in cases:
        got = C(F)
        assert got.dtype == np.float32 and got == f32(want), (F, got, want)
    assert C(F8(*[0.5] * 8)) == f32(1) - f32(2.0 ** -8) - f32(2.0 ** -8)
    # the position of the odd corner does not matter where every product is exact
    for c in range(8):
        F = np.ones(8, np.float32)
        F[c] = 0.5
        assert C(F) == f32(0.5)
        F = np.zeros(8, np.float32)
        F[c] = 1.0
        assert C(F) == f32(1.0)


def test_arrays_of_corners():
    """the corners are the leading axis; any shape follows"""
    rng = np.random.default_rng(1301)
    F = rng.random((8, 5, 7)).astype(np.float32)
    s = C(F)
    assert s.shape == (5, 7) and s.dtype == np.float32
    for i in range(5):
        for j in range(7):
            assert s[i, j] == C(F[:, i, j])
    want = 1.0 - np.prod(F.astype(np.float64), 0) - np.prod(1.0 - F.astype(np.float64), 0)
    assert np.max(np.abs(s - want)) < 1e-6  # the textbook formula, in double
    assert C(F, ax="not read").tobytes() == s.tobytes()  # the filter weights are not used


def test_a_subnormal_F_is_kept():
    """F_0 = 2^-140 is subnormal; lo = F_0 * 1 * 2^100 * 2^39 = 0.5 only if it is kept
    (flushed to zero, lo would be 0 and s would be 1).  hi = 1 * 0 * ... = 0."""
    t = f32(2.0 ** -140)
    assert 0 < t < np.finfo(np.float32).tiny
    F = F8(t, 1, 2.0 ** 100, 2.0 ** 39, 1, 1, 1, 1)
    assert C(F) == f32(0.5)
    # a product that becomes subnormal is kept as well: lo = 2^-130, then * 2^100 * 2^29
    F = F8(2.0 ** -65, 2.0 ** -65, 1, 2.0 ** 100, 2.0 ** 29, 1, 1, 1)
    assert f32(2.0 ** -65) * f32(2.0 ** -65) < np.finfo(np.float32).tiny
    assert C(F) == f32(0.5)
    # and nothing is clamped: an F outside [0, 1] gives what the lines give
    assert C(F8(2, 1, 1, 1, 1, 1, 1, 1)) == f32(-1.0)


def _scalar_left_to_right(F):
    lo, hi = F[0], f32(1) - F[0]
    for c in range(1, 8):
        lo = f32(lo * F[c])
        hi = f32(hi * f32(f32(1) - F[c]))
    return f32(f32(f32(1) - lo) - hi)


def _scalar_pairwise(F):
    def tree(v):
        while len(v) > 1:
            v = [f32(v[i] * v[i + 1]) for i in range(0, len(v), 2)]
        return v[0]
    lo = tree([f32(x) for x in F])
    hi = tree([f32(f32(1) - x) for x in F])
    return f32(f32(f32(1) - lo) - hi)


def test_the_multiplication_order_is_the_stated_one():
    """among seeded random corner sets (F in [0.8, 1): lo is of order 0.4, so its
    last bits reach s) some give other bits when the products are taken as a
    pairwise tree; the combine gives the left-to-right bits on all of them, and on
    the first that tells the two orders apart"""
    rng = np.random.default_rng(1302)
    found = None
    for _ in range(200):
        F = (rng.random(8) * 0.2 + 0.8).astype(np.float32)
        a, b = _scalar_left_to_right(F), _scalar_pairwise(F)
        assert C(F).view(np.uint32) == a.view(np.uint32), F
        if found is None and a.view(np.uint32) != b.view(np.uint32):
            found = F
    assert found is not None, "no corner set told the orders apart"
    assert C(found).view(np.uint32) != _scalar_pairwise(found).view(np.uint32)
    # reversing the corners is another order too, for some set
    assert any(C(F).tobytes() != C(F[::-1]).tobytes()
               for F in (rng.random((200, 8)) * 0.2 + 0.8).astype(np.float32))


def test_s_may_be_slightly_negative():
    """nothing is clamped: records that sum to a little more than 1 (f16 rounding
    does that) give F a little above 1, lo above 1 and s below 0; the transfer
    function clamps its argument, so such a sample is a sample of 0"""
    F = np.full(8, f32(1) + f32(2.0 ** -20), np.float32)
    s = C(F)
    assert -1e-5 < s < 0
    assert np.array_equal(ref_crossing.transfer(s), ref_crossing.transfer(f32(0)))
    # the f16 volumes of the GPU tests hold such cells
    Fh = cdf(DIMS, 8, "f16")
    assert Fh.max() > 1
    cells = np.stack([Fh[z:z + 15, y:y + 19, x:x + 23] for z in (0, 1) for y in (0, 1)
                      for x in (0, 1)])
    assert C(cells).min() < 0


# ---- the restated march loop ----

def camera(cam):
    pkg = graft.load_package()
    if cam == "C0":
        return pkg.camera.single_test_inv_view()
    return pkg.camera.display_inv_view((0.0, 90.0) if cam == "S" else (30.0, 45.0))


@functools.lru_cache(maxsize=None)
def volume(dims, nb, dtype):
    """the synthetic records of the tests, "f32" or narrowed to "f16"; read-only"""
    v = graft.load_oracle().synth_volume(*dims, nb)
    if dtype == "f16":
        v = v.astype(np.float16)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def weights(nb, theta=THETA):
    """the crossing weights of the isovalue: range_weights(0, theta, nb)"""
    w = graft.load_package().range_weights(0.0, theta, nb)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def cdf(dims, nb, dtype):
    """the plane of F of a volume at THETA, (nz, ny, nx) float32; read-only"""
    F = ref_crossing.cdf_plane(volume(dims, nb, dtype), weights(nb))
    F.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def reference(dims, nb, dtype, cam, w, h):
    """the numpy frame, computed once per case and shared by the CPU and the GPU
    tests: (RGBA8, float RGBA, samples, info), arrays read-only"""
    info = {}
    ref = ref_crossing.render_plane(cdf(dims, nb, dtype), w, h, camera(cam), info=info)
    for a in ref:
        a.setflags(write=False)
    return ref + (info,)


def test_the_loop_with_the_trilinear_blend_is_ref_weighted(orc):
    """what makes the restated loop trustworthy: with the trilinear blend for the
    combine it reproduces ref_weighted.render (ref_numpy._render with the weighted
    statistic) bit for bit, on an oblique view"""
    vol = volume(DIMS, 8, "f32")
    w = ref_weighted.seeded_weights(8)
    m = camera("C1")
    want = ref_weighted.render(vol, w, W, H, m)
    got = ref_crossing.render_plane(ref_weighted.lin_stat(vol, w), W, H, m,
                                    blend=ref_crossing.trilinear)
    hit = want[2] >= 0
    assert hit.sum() > 500 and np.unique(want[0][hit]).size > 100
    for g, r in zip(got, want):
        assert g.dtype == r.dtype and np.array_equal(g, r)
    # and the combine gives another frame on the same rays
    cross = ref_crossing.render(vol, w, W, H, m)
    assert not np.array_equal(cross[1], want[1])


def test_F_reaches_subnormal_values():
    """the synthetic records hold bins small enough for F to be subnormal at THETA"""
    for dims, nb in ((SMALL, 4), (DIMS, 8), (BAKE, 4)):
        F = cdf(dims, nb, "f32")
        sub = (F > 0) & (F < np.finfo(np.float32).tiny)
        assert sub.any(), (dims, nb, F[F > 0].min())
        assert F.min() >= 0 and F.max() <= f32(1.0001)


# the frames the GPU tests compare against: (dims, nb, dtype, view, width, height)
GPU_FRAMES = (
    [(SMALL, nb, dt, "C0", W, H) for nb in BINS for dt in ("f32", "f16")]
    + [(DIMS, 8, dt, cam, w, h) for dt in ("f32", "f16")
       for cam, w, h in (("C0", W, H), ("C1", W, H), ("S", W, H), ("C1", 70, 50))]
    + [(BAKE, 4, dt, cam, W, H) for dt in ("f32", "f16") for cam in ("C0", "C1", "S")]
)


@pytest.mark.parametrize("case", GPU_FRAMES, ids=lambda c: "-".join(
    "x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c))
def test_reference_frame_is_worth_comparing(case):
    """every reference frame of the GPU tests, by the reference alone: hit pixels of
    more than one colour, samples taken in cells the volume's edge clamps (a
    coincident corner enters twice there), and -- except for 2-bin records, whose F
    at 0.3 is too uniform to saturate a ray -- pixels that end early"""
    rgba8, _, n, info = reference(*case)
    hit = n >= 0
    colours = np.unique(rgba8[hit] & 0x00FFFFFF).size
    early = int(info["early"].sum())
    print(f"{int(hit.sum())} hit, {colours} colours, {early} early, "
          f"{info['clamped']} of {info['samples']} samples in clamped cells")
    assert hit.sum() > 20 and colours > 1, (case, int(hit.sum()), colours)
    assert info["clamped"] > 0 and info["clamped"] < info["samples"]
    if case[1] != 2:
        assert early > 0 and early < hit.sum()


# ---- host state of the C ABI ----

@pytest.mark.parametrize("nb", BINS)
def test_isovalue_weights_are_range_weights(pkg, nb):
    """bit for bit the weights of vr_set_query_range(0, theta, n); a theta below 0
    gives the all-zero weights of theta = 0 (range_weights refuses lo > hi)"""
    for theta in (-0.1, 0.0, 0.3, 0.5, 1.0, 1.5):
        pkg.set_isovalue(theta, nb)
        got = pkg.crossing_weights()
        want = pkg.range_weights(0.0, max(theta, 0.0), nb)
        assert got.dtype == np.float32 and got.size == nb
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (theta, got, want)
        if theta <= 0:
            assert not got.any()
        if theta >= 1:
            assert np.all(got == 1)
        if theta > 0:  # and through the C call itself
            pkg.set_query_range(0.0, theta, nb)
            assert np.array_equal(pkg.bin_weights().view(np.uint32), got.view(np.uint32))
    pkg.set_bin_weights(None)
    pkg.set_crossing_weights(None)


def test_crossing_state_without_gpu(pkg):
    L = pkg._lib.load()
    lib = pkg._lib
    pkg.freeCudaBuffers()
    pkg.set_crossing_weights(None)
    with pytest.raises(pkg.VRError) as e:
        pkg.crossing_weights()
    assert e.value.status == lib.VR_ERR_STATE
    # set, read back, replace
    for nb in BINS:
        w = (np.arange(nb, dtype=np.float32) - f32(1.5)) / f32(nb)
        pkg.set_crossing_weights(w)
        got = pkg.crossing_weights()
        assert np.array_equal(got, w) and got.dtype == np.float32
    # NULL arguments
    n = ctypes.c_int(-1)
    assert L.vr_crossing_weights(None, ctypes.addressof(n)) == lib.VR_OK and n.value == 32
    assert L.vr_crossing_weights(None, None) == lib.VR_OK
    # errors leave the state as it was
    keep = f32([0.125, -0.5, 2.25, 0.0])
    pkg.set_crossing_weights(keep)

    def unchanged():
        return np.array_equal(pkg.crossing_weights().view(np.uint32), keep.view(np.uint32))

    for n_bad in (0, 3, 5, 6, 12, 33, 64, -1):
        b = np.zeros(max(n_bad, 1), np.float32)
        assert L.vr_set_crossing_weights(b.ctypes.data, n_bad) == lib.VR_ERR_UNSUPPORTED
        assert unchanged()
        assert L.vr_set_isovalue(0.3, n_bad) == lib.VR_ERR_UNSUPPORTED
        assert unchanged()
    for bad in (float("nan"), float("inf"), float("-inf")):
        b = f32([0.5, bad])
        assert L.vr_set_crossing_weights(b.ctypes.data, 2) == lib.VR_ERR_ARG
        assert unchanged()
        assert L.vr_set_isovalue(bad, 4) == lib.VR_ERR_ARG
        assert unchanged()
    # no plane, and nothing to bake, without a volume
    assert pkg.crossing_info() == (None, 0)
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_crossing()
    assert e.value.status == lib.VR_ERR_STATE
    pkg.release_crossing()
    assert unchanged()  # releasing the plane keeps the weights
    pkg.freeCudaBuffers()
    assert unchanged()  # and so does freeCudaBuffers
    pkg.set_crossing_weights(None)
    with pytest.raises(pkg.VRError) as e:
        pkg.crossing_weights()
    assert e.value.status == lib.VR_ERR_STATE
    with pytest.raises(pkg.VRError) as e:  # nothing set and no volume
        pkg.bake_crossing()
    assert e.value.status == lib.VR_ERR_STATE
    L.vr_clear_error()


def test_crossing_state_is_apart_from_the_other_queries(pkg):
    pkg.set_bin_weights([1.0, 2.0])
    pkg.set_quantile(0.5)
    pkg.set_query_target([0.5, 0.5], "ks")
    pkg.set_crossing_weights([0.25, 0.75])
    assert np.array_equal(pkg.bin_weights(), f32([1.0, 2.0]))  # method 10's own weights
    pkg.set_bin_weights(None)
    pkg.set_quantile(None)
    pkg.set_query_target(None)
    assert np.array_equal(pkg.crossing_weights(), f32([0.25, 0.75]))
    pkg.set_bin_weights([1.0, 2.0])
    pkg.set_quantile(0.25)
    pkg.set_query_target([0.5, 0.5], "ks")
    pkg.set_isovalue(0.5, 4)
    assert np.array_equal(pkg.bin_weights(), f32([1.0, 2.0]))
    pkg.set_crossing_weights(None)
    assert np.array_equal(pkg.bin_weights(), f32([1.0, 2.0]))
    assert pkg.quantile() == (0.25, 0.25, False)
    got = pkg.query_target()
    assert np.array_equal(got[0], f32([0.5, 0.5])) and got[1:] == ("ks", False)
    pkg.set_bin_weights(None)
    pkg.set_quantile(None)
    pkg.set_query_target(None)


def test_render_method_13_without_volume(pkg):
    L = pkg._lib.load()
    pkg.freeCudaBuffers()
    pkg.set_isovalue(0.3, 2)
    d = pkg.make_desc(0x1000, W, H, pkg.camera.single_test_inv_view(),
                      query_method=pkg.QUERY_CROSSING, volume_size=(4, 4, 4))
    assert pkg.QUERY_CROSSING == 13 and pkg._lib.VR_QUERY_CROSSING == 13
    assert L.vr_render(ctypes.byref(d)) == pkg._lib.VR_ERR_STATE
    with pytest.raises(pkg.VRError) as e:
        pkg.render_kernel((4, 12, 1), (16, 4, 1), 0x1000, W, H, 0.05, 1.0, 0.0, 1.0, 13, (4, 4, 4))
    assert e.value.status == pkg._lib.VR_ERR_STATE
    assert L.vr_count_footprint(ctypes.byref(d)) == pkg._lib.VR_ERR_UNSUPPORTED
    assert L.vr_footprint_bytes(ctypes.byref(d)) == pkg._lib.VR_ERR_UNSUPPORTED
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_crossing()
    assert e.value.status == pkg._lib.VR_ERR_STATE
    # no GMM volume either: the state error comes first
    with pytest.raises(pkg.VRError) as e:
        pkg.render_gmm_baked(d)
    assert e.value.status == pkg._lib.VR_ERR_STATE
    L.vr_clear_error()
    pkg.set_crossing_weights(None)


def test_exports(pkg):
    for name in ("QUERY_CROSSING", "set_crossing_weights", "crossing_weights", "set_isovalue",
                 "bake_crossing", "release_crossing", "crossing_info"):
        assert name in pkg.api.__all__ and hasattr(pkg, name), name
    for name in ("vr_set_crossing_weights", "vr_crossing_weights", "vr_set_isovalue",
                 "vr_bake_crossing", "vr_release_crossing", "vr_crossing_info"):
        assert name in pkg._lib.EXPORTS and hasattr(pkg._lib.load(), name), name
