"""The range probability of GMM volumes (query method 10 on a GMM volume,
DESIGN.md section 18) without a GPU: the table of E = Phi - 1/2 the kernels read,
the numpy restatement of the statistic (ref_gmm_range) and its frame harness,
and the host state of the C ABI (vr_set_gmm_range and friends make no device
call)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import ref_gmm_range as ref

f32 = np.float32
INF = float("inf")
DIMS = (37, 11, 9)
W, H = 80, 64
BOUND_E = 2.0 ** -18       # the table against the true E, every float z
BOUND_P = 2.0 ** -16       # a voxel's probability against the true one, sum w = 1


def cam(pkg, name):
    return pkg.camera.single_test_inv_view() if name == "C0" else \
        pkg.camera.display_inv_view((30.0, 45.0))


@functools.lru_cache(maxsize=None)
def table(pkg):
    return pkg.gmm_phi_table()


@functools.lru_cache(maxsize=None)
def records(orc, K):
    wm, sg = orc.synth_gmm(*DIMS, K, seed=K)
    wm.setflags(write=False)
    sg.setflags(write=False)
    return wm, sg


def true_e(z):
    return np.array([0.5 * math.erf(float(v) / math.sqrt(2.0)) for v in np.ravel(z)]).reshape(
        np.shape(z))


# ---- the frame harness is the oracle's GMM march ----

@pytest.mark.parametrize("K", [8, 16])
def test_plane_harness_equals_the_oracle(pkg, orc, K):
    """ref_numpy.render over a plane of orc.gmm_stat (the mean) is orc.render_gmm,
    bit for bit: samples per pixel, packed RGBA8 and float RGBA, two cameras"""
    wm, sg = records(orc, K)
    X, Y, Z = DIMS
    plane = np.zeros((Z, Y, X), np.float32)
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                plane[z, y, x] = orc.gmm_stat(wm[z, y, x], sg[z, y, x], 1)
    for c in ("C0", "C1"):
        m = cam(pkg, c)
        want = orc.render_gmm(wm, sg, DIMS, orc.make_params(W, H, m, query_method=1))
        got = ref.render_plane(plane, W, H, m)
        assert (want["out_n"] > 0).any() and (want["out_n"] == -1).any()
        for key in ("out_n", "out", "out_f"):
            assert np.array_equal(got[key], want[key]), (K, c, key)


# ---- the table ----

def test_table_shape_and_constants(pkg):
    c, nseg, h, zmax = table(pkg)
    assert c.dtype == np.float32 and c.shape == (4, nseg + 1)
    assert nseg * h == zmax and math.frexp(h)[0] == 0.5   # h a power of two
    assert np.array_equal(c[:, nseg], f32([0.5, 0, 0, 0]))  # the row the clamp reads
    assert c[0, 0] == 0
    assert np.isfinite(c).all()


def test_table_accuracy(pkg):
    """|E - erf(z / sqrt 2) / 2| <= 2^-18 on a dense grid of [-7, 7], at every segment
    edge and the floats on either side of it, and beyond ZMAX"""
    c, nseg, h, zmax = tab = table(pkg)
    grid = np.linspace(-7.0, 7.0, 400001).astype(np.float32)
    edges = (np.arange(nseg + 1, dtype=np.float64) * h).astype(np.float32)
    around = np.concatenate([edges, np.nextafter(edges, f32(-1)), np.nextafter(edges, f32(9))])
    far = f32([zmax, 5.5, 8.0, 37.0, 1e6, 3e38])
    z = np.concatenate([grid, around, -around, far, -far])
    err = np.abs(ref.phi_e(z, tab).astype(np.float64) - true_e(z))
    worst = int(np.argmax(err))
    print(f"max |E - E_true| = {err[worst]:.3e} at z = {z[worst]!r}")
    assert err.max() <= BOUND_E, (err[worst], z[worst])


def test_table_is_odd_and_exact_at_its_ends(pkg):
    tab = table(pkg)
    rng = np.random.default_rng(18)
    z = np.concatenate([rng.normal(0, 3, 20000), [0.0, 1e-30, 1e-45, 4.9999995, 5.0, 7.0]]).astype(
        np.float32)
    pos, neg = ref.phi_e(z, tab), ref.phi_e(-z, tab)
    assert np.array_equal((-pos).view(np.uint32), neg.view(np.uint32))
    e = ref.phi_e(f32([0.0, -0.0, INF, -INF, 5.0, -5.0]), tab)
    assert np.array_equal(e.view(np.uint32), f32([0.0, -0.0, 0.5, -0.5, 0.5, -0.5]).view(np.uint32))


# ---- the statistic ----

def _one(K, w, mu, sd):
    """a record of K components: the given ones first, then zero weights"""
    wm = np.zeros((K, 2), np.float32)
    sg = np.full(K, 0.01, np.float32)
    n = len(w)
    wm[:n, 0], wm[:n, 1], sg[:n] = w, mu, sd
    return wm, sg


def canonical_sum(t):
    """four in order per lane, then the pairwise tree, float32"""
    t = np.asarray(t, dtype=np.float32).reshape(-1, 4)
    p = t[:, 0]
    for j in (1, 2, 3):
        p = p + t[:, j]
    while p.size > 1:
        p = p[0::2] + p[1::2]
    return p[0]


@pytest.mark.parametrize("K", [8, 16, 32])
def test_known_answers(pkg, K):
    tab = table(pkg)
    rs = ref.range_stat
    # one component of weight 1: half its mass lies below its mean, whatever sigma
    for mu, sd, at in ((0.3, 0.02, 0), (0.71, 3.0, K - 1), (-4.0, 1e-3, 5)):
        wm, sg = _one(K, [], [], [])
        wm[at], sg[at] = (1.0, mu), sd
        assert rs(wm, sg, -INF, f32(mu), tab) == f32(0.5)
        assert rs(wm, sg, f32(mu), INF, tab) == f32(0.5)
    # (-inf, +inf): every component counts whole -- the canonical sum of the weights
    rng = np.random.default_rng(K)
    wm = rng.random((K, 2)).astype(np.float32)
    sg = (0.005 + 0.05 * rng.random(K)).astype(np.float32)
    sg[3] = 0                                          # a Dirac counts whole too
    got = rs(wm, sg, -INF, INF, tab)
    assert got.view(np.uint32) == canonical_sum(wm[:, 0]).view(np.uint32)
    # a Dirac at 0.3 is inside [0.3, 0.4) and outside [0.2, 0.3)
    wm, sg = _one(K, [1.0], [0.3], [0.0])
    assert rs(wm, sg, 0.3, 0.4, tab) == 1 and rs(wm, sg, 0.2, 0.3, tab) == 0
    assert rs(wm, sg, -INF, 0.3, tab) == 0 and rs(wm, sg, 0.3, INF, tab) == 1
    # an empty range
    wm = rng.random((50, K, 2)).astype(np.float32)
    sg = (0.005 + 0.05 * rng.random((50, K))).astype(np.float32)
    for x in (0.0, 0.37, -2.0, INF, -INF):
        assert not rs(wm, sg, x, x, tab).any()


@pytest.mark.parametrize("K", [8, 16, 32])
def test_random_mixtures_against_double(pkg, K):
    """sum w = 1: within 2^-16 of sum w (Phi(zh) - Phi(zl)) in double with math.erf"""
    tab = table(pkg)
    rng = np.random.default_rng(100 + K)
    n = 400
    w = rng.random((n, K)) + 0.05
    w = (w / w.sum(-1, keepdims=True)).astype(np.float32)
    mu = rng.random((n, K)).astype(np.float32)
    sg = (10.0 ** rng.uniform(-3, 0.5, (n, K))).astype(np.float32)
    wm = np.stack([w, mu], -1)
    worst = 0.0
    for lo, hi in ((0.25, 0.75), (0.4, 0.5), (0.5, INF), (-INF, 0.3), (0.5, 0.5009765625)):
        got = ref.range_stat(wm, sg, lo, hi, tab).astype(np.float64)
        lo64, hi64 = float(f32(lo)), float(f32(hi))
        zh = (hi64 - mu.astype(np.float64)) / sg.astype(np.float64)
        zl = (lo64 - mu.astype(np.float64)) / sg.astype(np.float64)
        want = np.sum(w.astype(np.float64) * (true_e(zh) - true_e(zl)), -1)
        worst = max(worst, float(np.max(np.abs(got - want))))
    print(f"K={K}: max |P - P_true| = {worst:.3e}")
    assert worst <= BOUND_P


def test_f16_records_are_widened(pkg, orc):
    tab = table(pkg)
    wm, sg = records(orc, 8)
    hwm, hsg = wm[:2].astype(np.float16), sg[:2].astype(np.float16)
    a = ref.range_stat(hwm, hsg, 0.25, 0.75, tab)
    b = ref.range_stat(hwm.astype(np.float32), hsg.astype(np.float32), 0.25, 0.75, tab)
    assert np.array_equal(a, b) and not np.array_equal(a, ref.range_stat(wm[:2], sg[:2], 0.25, 0.75, tab))


# ---- the frames the GPU tests compare against ----

def test_reference_frame_takes_both_exits(pkg, orc):
    """[0.25, 0.75) at density 0.6 from C0: rays that stop on opacity > 0.95 and rays
    that leave the box -- against the frame at density 0, where no ray can turn
    opaque, the first take fewer samples and the second exactly as many"""
    wm, sg = records(orc, 16)
    plane = ref.range_stat(wm, sg, 0.25, 0.75, table(pkg))
    m = cam(pkg, "C0")
    fr = ref.render_plane(plane, W, H, m, density=0.6)
    box = ref.render_plane(plane, W, H, m, density=0.0)
    n, n_box, alpha = fr["out_n"], box["out_n"], fr["out_f"][..., 3]
    hit = n_box >= 0
    assert np.array_equal(n >= 0, hit) and hit.any() and (~hit).any()
    assert np.all(n[hit] <= n_box[hit]) and np.all(n_box[hit] < 500)
    early = hit & (n < n_box)
    through = hit & (n == n_box) & (alpha <= 0.95)
    print(f"rays: {int(hit.sum())} hit, {int(early.sum())} end on opacity, "
          f"{int(through.sum())} leave the box")
    assert early.sum() >= 1 and through.sum() >= 1


@pytest.mark.parametrize("rng", [(0.25, 0.75), (0.4, 0.5), (0.5, INF)])
def test_reference_frames_are_varied(pkg, orc, rng):
    """the synthetic volume (sigma in 0.005 .. 0.055) gives frames of many colours,
    not a constant 0 or 1: a wrong bound or a wrong sigma would show"""
    wm, sg = records(orc, 16)
    assert 0.005 <= sg.min() and sg.max() <= 0.055
    plane = ref.range_stat(wm, sg, *rng, table(pkg))
    assert plane.min() >= -1e-6 and plane.max() <= 1 + 1e-6
    assert plane.max() - plane.min() > 0.5
    out = ref.render_plane(plane, W, H, cam(pkg, "C1"))["out"]
    distinct = np.unique(out).size
    print(f"{rng}: {distinct} distinct RGBA8 values")
    assert distinct >= 340


# ---- host state, no GPU ----

def test_range_state_without_gpu(pkg):
    L = pkg._lib.load()
    E = pkg._lib
    pkg.freeCudaBuffers()
    pkg.clear_gmm_range()
    with pytest.raises(pkg.VRError) as e:
        pkg.gmm_range()
    assert e.value.status == E.VR_ERR_STATE
    pkg.set_gmm_range(0.25, 0.75)
    assert pkg.gmm_range() == (0.25, 0.75)
    pkg.set_gmm_range(0.3, INF)
    assert pkg.gmm_range() == (float(f32(0.3)), INF)
    pkg.set_gmm_range(-INF, 0.5)
    assert pkg.gmm_range() == (-INF, 0.5)
    pkg.set_gmm_range(-INF, INF)
    pkg.set_gmm_range(0.5, 0.5)
    # refused bounds keep the state
    for lo, hi in ((0.75, 0.25), (float("nan"), 0.5), (0.1, float("nan")), (INF, -INF)):
        assert L.vr_set_gmm_range(lo, hi) == E.VR_ERR_ARG
        assert pkg.gmm_range() == (0.5, 0.5)
    lo = ctypes.c_float(-1)
    assert L.vr_gmm_range(ctypes.addressof(lo), None) == E.VR_OK and lo.value == 0.5
    # no plane, and nothing to bake, without a volume
    assert pkg.gmm_range_info() == ((0, 0, 0), None, 0, 0)
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_gmm_range()
    assert e.value.status == E.VR_ERR_STATE
    pkg.release_gmm_range()
    assert pkg.gmm_range() == (0.5, 0.5)  # releasing the plane keeps the range
    pkg.clear_gmm_range()
    with pytest.raises(pkg.VRError) as e:
        pkg.gmm_range()
    assert e.value.status == E.VR_ERR_STATE
    L.vr_clear_error()


def test_method_10_without_volume_or_plane(pkg):
    L = pkg._lib.load()
    E = pkg._lib
    pkg.freeCudaBuffers()
    assert pkg.QUERY_WEIGHTED == 10
    d = pkg.make_desc(0x1000, W, H, pkg.camera.single_test_inv_view(), query_method=10,
                      volume_size=(1, 1, 1))
    for with_range in (False, True):
        if with_range:
            pkg.set_gmm_range(0.25, 0.75)
        else:
            pkg.clear_gmm_range()
        assert L.vr_render_gmm(ctypes.byref(d), None) == E.VR_ERR_STATE      # no volume
        assert L.vr_render_gmm_baked(ctypes.byref(d)) == E.VR_ERR_STATE      # no range plane
        assert L.vr_bake_gmm_range() == E.VR_ERR_STATE
    d3 = pkg.make_desc(0x1000, W, H, pkg.camera.single_test_inv_view(), query_method=3,
                       volume_size=(1, 1, 1))
    assert L.vr_render_gmm_baked(ctypes.byref(d3)) == E.VR_ERR_UNSUPPORTED   # as before
    L.vr_clear_error()
    pkg.clear_gmm_range()
