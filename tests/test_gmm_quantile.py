"""The quantile of GMM volumes (query method 11 on a GMM volume, DESIGN.md section
19) without a GPU: the host state of the C ABI (no call here touches a device),
known answers and the accuracy of the numpy restatement of the statistic
(ref_gmm_quantile), and its frame harness."""
import ctypes
import functools

import numpy as np
import pytest

import ref_gmm_quantile as ref
from ref_gmm_range import render_plane

f32 = np.float32
W, H = 80, 64
QS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.99, 1.0)
ULP = 2.0 ** -23           # one rounding of a midpoint of magnitude < 1 (see within())


@functools.lru_cache(maxsize=None)
def table(pkg):
    return pkg.gmm_phi_table()


@functools.lru_cache(maxsize=None)
def steps(pkg):
    return pkg.gmm_quantile_steps()


def one(K, w, mu, sd):
    """a record of K components: the given ones first, then zero weights at 0.5"""
    wm = np.zeros((K, 2), np.float32)
    wm[:, 1] = 0.5
    sg = np.full(K, 0.01, np.float32)
    n = len(w)
    wm[:n, 0], wm[:n, 1], sg[:n] = w, mu, sd
    return wm, sg


def Q(pkg, wm, sg, q):
    return ref.quantile_stat(wm, sg, q, q, False, table(pkg), steps(pkg))


def within(got, mu, width, n):
    """mu < got <= mu + width 2^-N: each bisection halves hi - lo and rounds the
    midpoint once, so the rounding adds at most one ulp of the values in all"""
    return mu < got <= mu + width * 2.0 ** -n + ULP


# ---- host state and ABI, no GPU ----

def test_steps_is_exported(pkg):
    assert pkg._lib.load().vr_gmm_quantile_steps() == 20 == pkg.gmm_quantile_steps()


def test_quantile_state_keeps_its_histogram_side_behaviour(pkg):
    L, E = pkg._lib.load(), pkg._lib
    pkg.freeCudaBuffers()
    pkg.set_quantile(None)
    with pytest.raises(pkg.VRError) as e:
        pkg.quantile()
    assert e.value.status == E.VR_ERR_STATE
    pkg.set_quantile(0.5)
    assert pkg.quantile() == (0.5, 0.5, False)
    pkg.set_quantile_spread(0.25, 0.75)
    assert pkg.quantile() == (0.25, 0.75, True)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        assert L.vr_set_quantile(bad) == E.VR_ERR_ARG
        assert pkg.quantile() == (0.25, 0.75, True)
    assert L.vr_set_quantile_spread(0.75, 0.25) == E.VR_ERR_ARG
    assert pkg.quantile() == (0.25, 0.75, True)
    pkg.set_quantile(1.0)
    assert pkg.quantile() == (1.0, 1.0, False)
    assert pkg.quantile_info() == (None, 0)          # the histogram-side plane: none
    assert L.vr_clear_quantile() == E.VR_OK
    with pytest.raises(pkg.VRError) as e:
        pkg.quantile()
    assert e.value.status == E.VR_ERR_STATE
    L.vr_clear_error()


def test_method_11_without_volume_or_plane(pkg):
    L, E = pkg._lib.load(), pkg._lib
    pkg.freeCudaBuffers()
    assert pkg.QUERY_QUANTILE == 11
    m = pkg.camera.single_test_inv_view()
    d = pkg.make_desc(0x1000, W, H, m, query_method=11, volume_size=(1, 1, 1))
    for q in (None, 0.5, (0.25, 0.75)):
        if isinstance(q, tuple):
            pkg.set_quantile_spread(*q)
        else:
            pkg.set_quantile(q)
        assert L.vr_bake_gmm_quantile() == E.VR_ERR_STATE              # no volume (and no quantile)
        assert L.vr_render_gmm(ctypes.byref(d), None) == E.VR_ERR_STATE
        assert L.vr_render_gmm_baked(ctypes.byref(d)) == E.VR_ERR_STATE  # no quantile plane
        assert pkg.gmm_quantile_info() == ((0, 0, 0), None, 0, 0)
        with pytest.raises(pkg.VRError) as e:
            pkg.bake_gmm_quantile()
        assert e.value.status == E.VR_ERR_STATE
    for method in (3, 7):
        dm = pkg.make_desc(0x1000, W, H, m, query_method=method, volume_size=(1, 1, 1))
        assert L.vr_render_gmm_baked(ctypes.byref(dm)) == E.VR_ERR_UNSUPPORTED   # as before
    pkg.release_gmm_quantile()                       # nothing to free: fine
    assert pkg.quantile() == (0.25, 0.75, True)      # releasing the plane keeps the quantile
    # any argument of the info call may be NULL
    n = ctypes.c_int(-1)
    assert L.vr_gmm_quantile_info(None, None, None, ctypes.addressof(n)) == E.VR_OK and n.value == 0
    pkg.set_quantile(None)
    L.vr_clear_error()


# ---- known answers of the reference ----

@pytest.mark.parametrize("K", [8, 16, 32])
def test_single_component_median(pkg, K):
    """one live component: the median is its mean, within 10 sigma 2^-N"""
    n = steps(pkg)
    for mu, sd, at in ((0.3, 0.02, 0), (0.71, 0.05, K - 1), (-4.0, 1e-3, 5), (0.5, 3.0, 2)):
        wm, sg = one(K, [], [], [])
        wm[at], sg[at] = (1.0, mu), sd
        got = float(Q(pkg, wm, sg, 0.5))
        width = 10.0 * float(f32(sd))
        assert abs(got - float(f32(mu))) <= width * 2.0 ** -n + abs(mu) * ULP, (mu, sd, got)


@pytest.mark.parametrize("K", [8, 16, 32])
def test_diracs(pkg, K):
    """0.25 each at 0.1, 0.3, 0.5, 0.7: Q steps from one to the next; the value is
    within (b0 - a0) 2^-N above the Dirac, and Q(1) is b0 itself"""
    n = steps(pkg)
    mus = f32([0.1, 0.3, 0.5, 0.7])
    wm, sg = one(K, [0.25] * 4, mus, [0.0] * 4)
    width = float(mus[3]) - float(mus[0])
    for q, k in ((0.25, 0), (0.3, 1), (0.75, 2)):
        got = float(Q(pkg, wm, sg, q))
        assert within(got, float(mus[k]), width, n), (q, got)
    assert Q(pkg, wm, sg, 1.0) == mus[3]
    # spread over the four components' lanes (K = 16: one per lane) it is the same
    if K >= 16:
        wm2, sg2 = one(K, [], [], [])
        for j in range(4):
            wm2[4 * j], sg2[4 * j] = (0.25, mus[j]), 0.0
        for q in (0.25, 0.3, 0.75, 1.0):
            assert Q(pkg, wm2, sg2, q) == Q(pkg, wm, sg, q)
    # a lone Dirac: the bracket is one point and every q gives it
    wm, sg = one(K, [1.0], [0.3], [0.0])
    for q in (0.0, 0.5, 1.0):
        assert Q(pkg, wm, sg, q) == f32(0.3)


@pytest.mark.parametrize("K", [8, 16, 32])
def test_no_positive_weight_gives_zero(pkg, K):
    wm, sg = one(K, [], [], [])
    for q in (0.0, 0.5, 1.0):
        got = Q(pkg, wm, sg, q)
        assert got == 0 and not np.signbit(got)
    got = ref.quantile_stat(wm, sg, 0.25, 0.75, True, table(pkg), steps(pkg))
    assert got == 0 and not np.signbit(got)
    wm[:, 0] = -0.25                                 # negative weights set no bracket either
    assert Q(pkg, wm, sg, 0.5) == 0


def test_separated_modes_hit_the_plateau(pkg):
    """two equal modes 60 sigma apart: the table CDF is exactly W / 2 on the gap
    between their supports, so the median search walks down to the plateau's lower
    end, the point where the lower mode's table value first reaches 1/2"""
    n, tab = steps(pkg), table(pkg)
    zmax = float(tab[3])
    wm, sg = one(16, [0.5, 0.5], [0.2, 0.8], [0.01, 0.01])
    mix = ref.Mixtures(wm, sg, tab)
    got = mix.quantile(0.5, n)
    assert got == Q(pkg, wm, sg, 0.5)                # deterministic
    lo_mode, sd = float(f32(0.2)), float(f32(0.01))
    assert lo_mode + 4.0 * sd < got <= lo_mode + zmax * sd + (float(mix.b0) - float(mix.a0)) * 2.0 ** -n + ULP
    assert float(f32(0.8)) - zmax * sd > got         # inside the gap
    assert mix.cdf(got) == f32(0.5) and mix.cdf(f32(0.5)) == f32(0.5)
    assert mix.cdf(np.nextafter(got, f32(-1)) - f32(2.0 ** -n)) < f32(0.5)


@pytest.mark.parametrize("K", [8, 16, 32])
def test_monotone_in_q(pkg, orc, K):
    """over fixed records Q never falls by more than one search step as q rises (the
    table dips by 1 ulp at some segment joints)"""
    n, tab = steps(pkg), table(pkg)
    wm, sg = orc.synth_gmm(6, 5, 4, K, seed=K)
    mix = ref.Mixtures(wm, sg, tab)
    step = (mix.b0.astype(np.float64) - mix.a0.astype(np.float64)) * 2.0 ** -n
    prev = mix.quantile(0.0, n)
    assert np.all(np.abs(prev.astype(np.float64) - mix.a0) <= step + ULP)   # Q(0): the lower edge
    for q in np.linspace(0.0, 1.0, 41)[1:]:
        cur = mix.quantile(q, n)
        assert np.all(cur.astype(np.float64) >= prev.astype(np.float64) - step), q
        prev = cur
    # Q(1): where the float CDF first rounds to W, at or a fraction of a sigma below b0
    gap = mix.b0.astype(np.float64) - prev
    print(f"K={K}: b0 - Q(1) <= {gap.max():.3e} = {np.max(gap / sg.max(-1)):.3f} sigma")
    assert np.all(gap >= 0) and np.all(gap <= sg.max(-1))


def test_spread_is_one_subtraction(pkg, orc):
    n, tab = steps(pkg), table(pkg)
    wm, sg = orc.synth_gmm(6, 5, 4, 16, seed=3)
    lo, hi = Q(pkg, wm, sg, 0.25), Q(pkg, wm, sg, 0.75)
    iqr = ref.quantile_stat(wm, sg, 0.25, 0.75, True, tab, n)
    assert iqr.dtype == np.float32 and np.array_equal(iqr.view(np.uint32), (hi - lo).view(np.uint32))
    assert np.all(iqr > 0)


def test_f16_records_are_widened(pkg, orc):
    n, tab = steps(pkg), table(pkg)
    wm, sg = orc.synth_gmm(6, 5, 2, 8, seed=8)
    hwm, hsg = wm.astype(np.float16), sg.astype(np.float16)
    a = ref.quantile_stat(hwm, hsg, 0.5, 0.5, False, tab, n)
    b = ref.quantile_stat(hwm.astype(np.float32), hsg.astype(np.float32), 0.5, 0.5, False, tab, n)
    assert np.array_equal(a, b) and not np.array_equal(a, Q(pkg, wm, sg, 0.5))


# ---- accuracy against the double-precision erf CDF ----

def true_cdf(w, mu, sd, x):
    import torch
    z = (x[..., None] - mu.astype(np.float64)) / (sd.astype(np.float64) * np.sqrt(2.0))
    e = torch.erf(torch.from_numpy(z)).numpy()
    return np.sum(w.astype(np.float64) * 0.5 * (1.0 + e), -1)


@pytest.mark.parametrize("K", [8, 16, 32])
def test_accuracy_against_double(pkg, orc, K):
    """10 000 mixtures of the synthetic volume: |F(Q) - q W| <=
    2^-16 + (b0 - a0) 2^-N sum_k w_k / (sigma_k sqrt(2 pi)) -- the table and the float
    sums, plus the search step times the largest possible density"""
    n, tab = steps(pkg), table(pkg)
    wm, sg = orc.synth_gmm(25, 20, 20, K, seed=100 + K)
    wm, sg = wm.reshape(-1, K, 2), sg.reshape(-1, K)
    assert wm.shape[0] == 10000
    mix = ref.Mixtures(wm, sg, tab)
    w, mu = wm[..., 0], wm[..., 1]
    dens = np.sum(w.astype(np.float64) / (sg.astype(np.float64) * np.sqrt(2.0 * np.pi)), -1)
    bound = 2.0 ** -16 + (mix.b0.astype(np.float64) - mix.a0) * 2.0 ** -n * dens
    worst, worst_abs = 0.0, 0.0
    for q in QS:
        got = mix.quantile(q, n).astype(np.float64)
        resid = np.abs(true_cdf(w, mu, sg, got) - float(f32(q)) * mix.W.astype(np.float64))
        ratio = resid / bound
        print(f"K={K} q={q}: max |F(Q) - q W| = {resid.max():.3e}, max ratio to the bound "
              f"{ratio.max():.3f}")
        worst, worst_abs = max(worst, float(ratio.max())), max(worst_abs, float(resid.max()))
    print(f"K={K}: largest ratio {worst:.3f}, largest residual {worst_abs:.3e}")
    assert worst <= 1.0


# ---- the frame harness ----

def test_frame_harness(pkg, orc):
    """a frame of the per-voxel statistic through ref_gmm_range.render_plane: the
    dict the GPU tests compare against, with hits, misses and many colours"""
    n, tab = steps(pkg), table(pkg)
    dims = (24, 20, 18)
    wm, sg = orc.synth_gmm(*dims, 16, seed=16)
    plane = ref.quantile_stat(wm, sg, 0.5, 0.5, False, tab, n)
    assert plane.shape == dims[::-1] and plane.dtype == np.float32
    assert plane.min() >= 0 and plane.max() <= 1 and plane.max() - plane.min() > 0.3
    m = pkg.camera.display_inv_view((30.0, 45.0))
    fr = render_plane(plane, W, H, m)
    assert set(fr) == {"out", "out_f", "out_n"}
    assert fr["out"].shape == (H, W) and fr["out"].dtype == np.uint32
    assert fr["out_f"].shape == (H, W, 4) and fr["out_f"].dtype == np.float32
    assert fr["out_n"].shape == (H, W) and fr["out_n"].dtype == np.int32
    assert (fr["out_n"] > 0).any() and (fr["out_n"] == -1).any()
    assert np.unique(fr["out"]).size >= 200
    again = ref.render(wm, sg, 0.5, 0.5, False, tab, n, W, H, m)
    for key in fr:
        assert np.array_equal(fr[key], again[key])
