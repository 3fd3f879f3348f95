"""The 2-D transfer function over two planes without a GPU:
known answers of the numpy classifier, its collapse to the 1-D classifier for 8-bit
tables (and not for float ones), the two-plane march restatement against the
one-plane loops bit for bit, the host state of the C ABI
(vr_set_transfer_function_2d makes no device call), and the reference frames the
GPU tests compare against."""
import ctypes
import functools

import numpy as np
import pytest

import __graft_entry__ as graft
import ref_crossing
import ref_numpy
import ref_quantile
import ref_transfer
import ref_transfer2
from test_crossing import BAKE, DIMS, H, W, camera, cdf, volume
from test_transfer import RAMP2, SPECIALS

f32 = np.float32
T2 = ref_transfer2.transfer_table2
CODEC = (22, 18, 14)  # orc.synth_codec(22, 18, 14, 8, seed=8)


# ---- the tables of the tests (read-only, shared with tests/test_gpu_transfer2.py) ----

def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


# (nv, nu, 4).  2 x 2: a blue-to-red opacity ramp along u whose opacity turns round
# along v; 32 x 32: every thread of the staging loop copies four entries; 255 x 4
# (nu x nv): the last staging round is partial; 1 x 1, 3 x 1 and 1 x 5: one axis
# without a second entry
RAMP22 = _ro([[(0, 0, 1, 0), (1, 0, 0, 1)], [(0, 1, 1, 1), (1, 1, 0, 0)]])
RAND32 = _ro(np.random.default_rng(1501).random((32, 32, 4)))
T255X4 = _ro(np.random.default_rng(1502).random((4, 255, 4)))
ONE = _ro([[(0.25, 0.5, 0.75, 0.5)]])
T3X1 = _ro(np.random.default_rng(1503).random((1, 3, 4)))
T1X5 = _ro(np.random.default_rng(1504).random((5, 1, 4)))
TABLES = {"ramp22": RAMP22, "rand32": RAND32, "t255x4": T255X4, "one": ONE, "t3x1": T3X1,
          "t1x5": T1X5}

# pair -> (u, v, v_offset, v_scale).  The v window is chosen from the range of v's
# plane on DIMS x 8 (percentiles 0 / 95): method 13's combine and method 10's F fill
# [0, 1]; the variance plane lies in [0.088, 0.41] (0.32 at 95 %); the median in
# [0.06, 0.94] (0.45 at 95 %); the codec entropy in [0.24, 0.98]
PAIRS = {"1-13": (1, 13, 0.0, 1.0), "13-2": (13, 2, 0.08, 3.0), "10-11": (10, 11, 0.05, 2.0),
         "10-10": (10, 10, 0.0, 1.0), "4-6": (4, 6, 0.2, 1.25)}
# the (pair, table) combinations the GPU tests render: every table and every pair
FRAMES = (("1-13", "ramp22"), ("1-13", "rand32"), ("13-2", "t255x4"), ("13-2", "one"),
          ("10-11", "t3x1"), ("10-11", "t1x5"), ("10-10", "rand32"), ("10-10", "t255x4"))


def blend_of(method):
    return ref_crossing.combine if method == 13 else ref_crossing.trilinear


@functools.lru_cache(maxsize=None)
def codec_records():
    cb, t, e = graft.load_oracle().synth_codec(*CODEC, 8, seed=8)
    return cb, t, e


@functools.lru_cache(maxsize=None)
def plane(dims, nb, dtype, method):
    """the baked plane of `method` as numpy computes it, (nz, ny, nx) float32,
    read-only: 1 / 2 ref_numpy.stat, 10 and 13 F at THETA (the GPU tests set the
    range [0, THETA) and the isovalue THETA), 11 the median; dims == CODEC: 4 / 5 / 6
    of the decoded codec records"""
    with np.errstate(all="ignore"):
        if method in (4, 5, 6):
            assert dims == CODEC
            p = ref_numpy.codec_stat(ref_numpy.codec_decode(*codec_records()), method - 4)
        elif method in (10, 13):
            p = cdf(dims, nb, dtype)
        else:
            v = np.asarray(volume(dims, nb, dtype)).astype(np.float32)
            p = (ref_quantile.quantile_stat(v, 0.5) if method == 11
                 else ref_numpy.stat(v, method - 1))
    p = np.ascontiguousarray(p, dtype=np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reference(pair, table, dims, nb, dtype, cam, w, h, row0=False):
    """the numpy frame of PAIRS[pair] under TABLES[table] (row0: with every row
    replaced by row 0), computed once per case and shared by the CPU and the GPU
    tests: (RGBA8, float RGBA, samples, info), arrays read-only"""
    u, v, voff, vscale = PAIRS[pair]
    tab = TABLES[table]
    if row0:
        tab = np.repeat(tab[:1], tab.shape[0], axis=0)
    info = {}
    ref = ref_transfer2.render_planes(plane(dims, nb, dtype, u), plane(dims, nb, dtype, v), w, h,
                                      camera(cam), tab, blend_u=blend_of(u), blend_v=blend_of(v),
                                      voff=voff, vscale=vscale, info=info)
    for a in ref:
        a.setflags(write=False)
    return ref + (info,)


# ---- known answers of transfer_table2 ----

def test_one_entry_is_constant():
    x = np.concatenate([np.linspace(-1, 2, 301, dtype=np.float32), SPECIALS])
    got = T2(x[:, None], x[None, :], ONE)
    assert got.dtype == np.float32 and got.shape == (x.size, x.size, 4)
    assert np.all(got == ONE[0, 0])  # 8-bit values: both lerps are exact


def test_two_by_two():
    """entry (i, j) is centred at ((i + 1/2) / nu, (j + 1/2) / nv)"""
    for j, xv in ((0, 0.25), (1, 0.75)):
        for i, xu in ((0, 0.25), (1, 0.75)):
            assert np.array_equal(T2(f32(xu), f32(xv), RAMP22), RAMP22[j, i])
    assert np.array_equal(T2(f32(0.5), f32(0.5), RAMP22), f32([0.5, 0.5, 0.5, 0.5]))
    assert np.array_equal(T2(f32(0.5), f32(0.25), RAMP22), f32([0.5, 0, 0.5, 0.5]))
    assert np.array_equal(T2(f32(0.25), f32(0.5), RAMP22), f32([0, 0.5, 1, 0.5]))
    # outside [0.25, 0.75] the clamped indices repeat an entry, on each axis
    for x in (0.0, 0.1, 0.2):
        assert np.array_equal(T2(f32(x), f32(0.75), RAMP22), RAMP22[1, 0]), x
        assert np.array_equal(T2(f32(0.75), f32(x), RAMP22), RAMP22[0, 1]), x
    for x in (0.8, 0.9, 1.0):
        assert np.array_equal(T2(f32(x), f32(0.25), RAMP22), RAMP22[0, 1]), x
        assert np.array_equal(T2(f32(0.25), f32(x), RAMP22), RAMP22[1, 0]), x


def test_the_weights_are_quantised_on_each_axis_by_itself():
    """x = 0.25 + d / 2 has the exact weight d; the table sees rint(256 d) / 256, along
    u whatever xv is and along v whatever xu is"""
    along_u = f32([[(0,) * 4, (256,) * 4]] * 2)
    along_v = f32([[(0,) * 4] * 2, [(256,) * 4] * 2])
    for d, q in ((1 / 256, 1), (1 / 512 + 1 / 4096, 1), (1 / 1024, 0), (100.3 / 256, 100),
                 (3 / 512, 2), (1 / 512, 0)):  # the last two: ties go to even
        for other in (0.0, 0.3, 0.5 + 1 / 1024, 1.0):
            got = T2(f32(0.25 + d / 2), f32(other), along_u)
            assert np.all(got == f32(q)), (d, q, other, got)
            got = T2(f32(other), f32(0.25 + d / 2), along_v)
            assert np.all(got == f32(q)), (d, q, other, got)


def test_clamping_on_each_axis():
    """x < 0 is x = 0, x > 1 is x = 1, -inf / +inf with them, NaN is 0"""
    for mid in (0.0, 0.37, 1.0):
        lo_u, hi_u = T2(f32(0), f32(mid), RAND32), T2(f32(1), f32(mid), RAND32)
        lo_v, hi_v = T2(f32(mid), f32(0), RAND32), T2(f32(mid), f32(1), RAND32)
        for x in (-1e-30, -0.5, -1e30, -np.inf, np.nan):
            assert np.array_equal(T2(f32(x), f32(mid), RAND32), lo_u), x
            assert np.array_equal(T2(f32(mid), f32(x), RAND32), lo_v), x
        for x in (1.0000001, 1.5, 1e30, np.inf):
            assert np.array_equal(T2(f32(x), f32(mid), RAND32), hi_u), x
            assert np.array_equal(T2(f32(mid), f32(x), RAND32), hi_v), x
    assert np.array_equal(T2(f32(0), f32(0), RAND32), RAND32[0, 0])
    assert np.array_equal(T2(f32(1), f32(0), RAND32), RAND32[0, 31])
    assert np.array_equal(T2(f32(0), f32(1), RAND32), RAND32[31, 0])
    # nothing in the table is clamped
    assert np.array_equal(T2(f32(0.5), f32(0.5), f32([[(-3, 7, 1e30, -0.0)]])),
                          f32([-3, 7, 1e30, 0]))


# ---- collapse to the 1-D classifier ----

def _xs():
    k = np.arange(-16384, 81921, dtype=np.int64)  # every k / 65536 in [-0.25, 1.25]
    xu = np.concatenate([(k.astype(np.float64) / 65536.0).astype(np.float32), SPECIALS])
    xv = np.concatenate([np.linspace(-0.25, 1.25, 17, dtype=np.float32), SPECIALS])
    assert xu[0] == f32(-0.25) and xu[k.size - 1] == f32(1.25)
    return xu, xv


@pytest.mark.parametrize("n", (256, 9))
def test_rows_of_one_8_bit_table_are_the_1d_classifier(pkg, n):
    """every value m / 256, 0 <= m <= 256: lerpq(r, r, b) = r exactly, so the 2-D
    result is the 1-D one byte for byte, for every nv and every xv"""
    t1 = (pkg.REFERENCE_TF if n == 9 else
          np.random.default_rng(1505).integers(0, 257, (n, 4)).astype(np.float32) / f32(256))
    xu, xv = _xs()
    want = ref_transfer.transfer_table(xu, t1)
    assert np.unique(want, axis=0).shape[0] > 1000
    for nv in (1, 2, 4):
        got = T2(xu[:, None], xv[None, :], np.repeat(t1[None], nv, axis=0))
        assert got.shape == (xu.size, xv.size, 4)
        for c in range(xv.size):
            assert got[:, c].tobytes() == want.tobytes(), (nv, xv[c])


def test_rows_of_one_float_table_do_not_collapse():
    """the premise of the test above: with arbitrary floats lerpq(r, r, b) != r for
    some (r, b), so the property is one of 8-bit tables only"""
    t1 = np.random.default_rng(1506).random((256, 4)).astype(np.float32)
    xu, xv = _xs()
    want = ref_transfer.transfer_table(xu, t1)
    got = T2(xu[:, None], xv[None, :], np.repeat(t1[None], 2, axis=0))
    differ = int((got != want[:, None, :]).sum())
    assert differ > 0
    assert np.allclose(got, want[:, None, :], rtol=0, atol=2e-7)  # the last bit only
    # where b is 0 the second lerp is 1 * r + 0 * r: exact
    assert np.array_equal(T2(xu, f32(0.25), np.repeat(t1[None], 2, axis=0)), want)


# ---- the march restatement ----

@pytest.mark.parametrize("blend", ("combine", "trilinear"))
def test_the_two_plane_march_is_the_one_plane_march(pkg, blend):
    """with both planes the same F and rows of one 8-bit table, render_planes is
    ref_transfer.render_plane (ref_crossing._march) bit for bit; with the reference's
    nine entries it is the built-in frame"""
    bl = {"combine": ref_crossing.combine, "trilinear": ref_crossing.trilinear}[blend]
    F, m = cdf(DIMS, 8, "f32"), camera("C1")
    t1 = np.random.default_rng(1507).integers(0, 257, (64, 4)).astype(np.float32) / f32(256)
    info_a, info_b = {}, {}
    want = ref_transfer.render_plane(F, W, H, m, t1, blend=bl, density=0.07, brightness=1.25,
                                     toff=0.05, tscale=1.5, info=info_a)
    other = ref_crossing.trilinear if blend == "combine" else ref_crossing.combine
    got = ref_transfer2.render_planes(F, F, W, H, m, np.repeat(t1[None], 3, axis=0), blend_u=bl,
                                      blend_v=other, voff=0.1, vscale=2.0, density=0.07,
                                      brightness=1.25, toff=0.05, tscale=1.5, info=info_b)
    assert (want[2] >= 0).sum() > 500
    for g, r in zip(got, want):
        assert g.dtype == r.dtype and np.array_equal(g, r)
    assert np.array_equal(info_a["early"], info_b["early"])
    assert (info_a["samples"], info_a["clamped"]) == (info_b["samples"], info_b["clamped"])
    base = ref_crossing.render_plane(F, W, H, m, blend=bl)
    got = ref_transfer2.render_planes(F, F, W, H, m, np.repeat(pkg.REFERENCE_TF[None], 3, axis=0),
                                      blend_u=bl, blend_v=other)
    for g, r in zip(got, base):
        assert g.dtype == r.dtype and np.array_equal(g, r)


# ---- host state of the C ABI ----

def _state(pkg):
    t = pkg.transfer_function_2d()
    return None if t is None else (t[0].tobytes(), t[0].shape) + t[1:]


def _set(L, tab, mv, off=0.0, scale=1.0):
    tab = np.ascontiguousarray(tab, dtype=np.float32)
    return L.vr_set_transfer_function_2d(tab.ctypes.data, tab.shape[1], tab.shape[0], mv, off,
                                         scale)


def test_transfer2_state_without_gpu(pkg):
    L, lib = pkg._lib.load(), pkg._lib
    assert lib.VR_TF2_MAX == pkg.TF2_MAX == 1024
    pkg.freeCudaBuffers()
    pkg.set_transfer_function(None)
    pkg.set_transfer_function_2d(None)
    L.vr_clear_error()
    assert pkg.transfer_function_2d() is None
    nu, nv = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.vr_transfer_function_2d(None, ctypes.addressof(nu), ctypes.addressof(nv), None, None,
                                     None) == lib.VR_OK
    assert (nu.value, nv.value) == (0, 0)
    assert L.vr_transfer_function_2d(None, None, None, None, None, None) == lib.VR_OK
    # set, read back, replace: (nu, nv)
    rng = np.random.default_rng(1508)
    for (a, b), mv in zip(((1, 1), (2, 2), (32, 32), (255, 4), (256, 1), (1, 256), (3, 5)),
                          (1, 2, 3, 4, 10, 12, 13)):
        tab = (rng.random((b, a, 4)) * 4 - 2).astype(np.float32)
        pkg.set_transfer_function_2d(tab, mv, v_offset=0.25 * a, v_scale=-1.5 * b)
        got = pkg.transfer_function_2d()
        assert got[0].dtype == np.float32 and got[0].shape == (b, a, 4)
        assert np.array_equal(got[0], tab) and got[1:] == (mv, 0.25 * a, -1.5 * b)
    pkg.set_transfer_function_2d([[[0, 0, 0, 0], [1, 1, 1, 1]]], 11)  # any array-like
    assert pkg.transfer_function_2d()[0].shape == (1, 2, 4)
    for shape in ((3, 4), (2, 3, 3), (4,)):
        with pytest.raises(ValueError):
            pkg.set_transfer_function_2d(np.zeros(shape, np.float32), 1)
    # errors leave the state as it was
    pkg.set_transfer_function_2d(RAMP22, 13, 0.5, 2.0)
    keep = _state(pkg)
    big = np.zeros(4 * 2048, np.float32)
    for a, b in ((1025, 1), (41, 25), (257, 1), (1, 257), (0, 1), (1, 0), (0, 0), (-1, 4), (4, -1),
                 (-2, -2), (1 << 16, 1 << 16)):
        assert L.vr_set_transfer_function_2d(big.ctypes.data, a, b, 1, 0.0, 1.0) == lib.VR_ERR_ARG
        assert _state(pkg) == keep, (a, b)
    for mv in (0, 7, 8, 9, 14, -1):
        assert _set(L, RAND32, mv) == lib.VR_ERR_ARG
        assert _state(pkg) == keep, mv
    for bad in (np.nan, np.inf, -np.inf):
        for where in ((0, 0, 0), (1, 1, 3), (31, 31, 2)):
            t = RAND32.copy()
            t[where] = bad
            with pytest.raises(pkg.VRError) as e:
                pkg.set_transfer_function_2d(t, 1)
            assert e.value.status == lib.VR_ERR_ARG and "finite" in str(e.value)
            assert _state(pkg) == keep
        assert _set(L, RAND32, 1, bad, 1.0) == lib.VR_ERR_ARG
        assert _state(pkg) == keep
        assert _set(L, RAND32, 1, 0.0, bad) == lib.VR_ERR_ARG
        assert _state(pkg) == keep
    # the table is the caller's: it outlives freeCudaBuffers, the other queries'
    # state and their planes' releases; nothing so far has made a device call
    L.vr_clear_error()
    pkg.freeCudaBuffers()
    pkg.release_stats()
    pkg.release_crossing()
    pkg.release_gmm_stats()
    pkg.set_bin_weights([1.0, 2.0])
    pkg.set_bin_weights(None)
    assert _state(pkg) == keep
    L.vr_clear_error()
    pkg.set_transfer_function_2d(T255X4, 2)
    assert L.vr_last_status() == lib.VR_OK and L.vr_last_error() == b""
    # only a NULL call clears it (the other arguments are not read)
    assert L.vr_set_transfer_function_2d(None, 77, -3, 99, float("nan"), float("inf")) == lib.VR_OK
    assert pkg.transfer_function_2d() is None


def test_at_most_one_of_the_two_tables_is_set(pkg):
    L, lib = pkg._lib.load(), pkg._lib
    pkg.set_transfer_function(None)
    pkg.set_transfer_function_2d(None)
    pkg.set_transfer_function(RAMP2)
    pkg.set_transfer_function_2d(RAMP22, 13)  # clears the 1-D table
    assert pkg.transfer_function() is None and pkg.transfer_function_2d() is not None
    pkg.set_transfer_function(RAMP2)          # and the other way round
    assert pkg.transfer_function_2d() is None and np.array_equal(pkg.transfer_function(), RAMP2)
    # a NULL call clears only its own table
    pkg.set_transfer_function_2d(None)
    assert np.array_equal(pkg.transfer_function(), RAMP2)
    pkg.set_transfer_function_2d(RAMP22, 13)
    pkg.set_transfer_function(None)
    assert pkg.transfer_function_2d() is not None
    # a refused call clears nothing
    assert L.vr_set_transfer_function(RAMP2.ctypes.data, 0) == lib.VR_ERR_ARG
    assert pkg.transfer_function_2d() is not None
    pkg.set_transfer_function_2d(None)
    pkg.set_transfer_function(RAMP2)
    assert _set(L, RAMP22, 7) == lib.VR_ERR_ARG
    assert np.array_equal(pkg.transfer_function(), RAMP2)
    pkg.set_transfer_function(None)
    L.vr_clear_error()


def test_refusals_come_before_any_device_work(pkg):
    """with a 2-D table set, what has no plane march is refused outright -- the counts
    before they look at their descriptor"""
    L, lib = pkg._lib.load(), pkg._lib
    pkg.freeCudaBuffers()
    pkg.set_transfer_function_2d(RAMP22, 13)
    try:
        d = pkg.make_desc(0x1000, W, H, camera("C0"), query_method=1, volume_size=(4, 4, 4))
        for call in (L.vr_count_footprint, L.vr_footprint_bytes, L.vr_gmm_count_footprint):
            assert call(ctypes.byref(d)) == lib.VR_ERR_UNSUPPORTED
            msg = L.vr_last_error().decode()
            assert "custom transfer function" in msg and "bake" in msg and "clear" in msg, msg
            assert "vr_set_transfer_function_2d" in msg
        assert L.vr_render_gmm(ctypes.byref(d), None) == lib.VR_ERR_UNSUPPORTED
        assert "custom transfer function" in L.vr_last_error().decode()
        # no baked GMM plane: the table's refusal, not a state error
        assert L.vr_render_gmm_baked(ctypes.byref(d)) == lib.VR_ERR_UNSUPPORTED
        assert "custom transfer function" in L.vr_last_error().decode()
    finally:
        pkg.set_transfer_function_2d(None)
        L.vr_clear_error()
    # cleared: the usual state errors of a library without a volume
    assert L.vr_count_footprint(ctypes.byref(d)) == lib.VR_ERR_STATE
    assert L.vr_render_gmm_baked(ctypes.byref(d)) == lib.VR_ERR_STATE
    L.vr_clear_error()


def test_exports(pkg):
    for name in ("TF2_MAX", "set_transfer_function_2d", "transfer_function_2d"):
        assert name in pkg.api.__all__ and hasattr(pkg, name), name
    for name in ("vr_set_transfer_function_2d", "vr_transfer_function_2d"):
        assert name in pkg._lib.EXPORTS and hasattr(pkg._lib.load(), name), name


# ---- the reference frames of the GPU tests ----

# (pair, table, view) -> (hit pixels, early endings) of the 64 x 48 frame of DIMS x 8
# f32 (pair "4-6": the codec volume), for every combination whose table has a v axis
PINNED = {
    ("1-13", "ramp22", "C0"): (1389, 403), ("1-13", "ramp22", "C1"): (1330, 412),
    ("1-13", "ramp22", "S"): (1389, 334),
    ("1-13", "rand32", "C0"): (1389, 702), ("1-13", "rand32", "C1"): (1330, 639),
    ("1-13", "rand32", "S"): (1389, 679),
    ("13-2", "t255x4", "C0"): (1389, 726), ("13-2", "t255x4", "C1"): (1330, 676),
    ("13-2", "t255x4", "S"): (1389, 717),
    ("10-11", "t1x5", "C0"): (1389, 914), ("10-11", "t1x5", "C1"): (1330, 916),
    ("10-11", "t1x5", "S"): (1389, 939),
    ("10-10", "rand32", "C0"): (1389, 845), ("10-10", "rand32", "C1"): (1330, 854),
    ("10-10", "rand32", "S"): (1389, 844),
    ("10-10", "t255x4", "C0"): (1389, 591), ("10-10", "t255x4", "C1"): (1330, 517),
    ("10-10", "t255x4", "S"): (1389, 589),
    ("4-6", "rand32", "C0"): (1389, 724), ("4-6", "rand32", "C1"): (1330, 677),
    ("4-6", "rand32", "S"): (1389, 715),
    ("4-6", "ramp22", "C0"): (1389, 717), ("4-6", "ramp22", "C1"): (1330, 649),
    ("4-6", "ramp22", "S"): (1389, 710),
}


@pytest.mark.parametrize("pair,table,cam", sorted(PINNED), ids=["-".join(k) for k in sorted(PINNED)])
def test_reference_frame_is_worth_comparing(pair, table, cam):
    """by the reference alone: more than 100 hit pixels of more than 50 colours, rays
    that end early and rays that run their full length, and a v axis that matters --
    the frame under the same table with every row replaced by row 0 differs in at
    least a quarter of the hit pixels"""
    dims = CODEC if pair == "4-6" else DIMS
    rgba8, _, n, info = reference(pair, table, dims, 8, "f32", cam, W, H)
    flat = reference(pair, table, dims, 8, "f32", cam, W, H, row0=True)
    hit = n >= 0
    colours = np.unique(rgba8[hit]).size
    early = int(info["early"].sum())
    differ = int((rgba8 != flat[0])[hit].sum())
    print(f"{int(hit.sum())} hit, {colours} colours, {early} early, {differ} differ from row 0")
    assert np.array_equal(hit, flat[2] >= 0)
    assert (int(hit.sum()), early) == PINNED[pair, table, cam]
    assert hit.sum() > 100 and colours > 50 and 0 < early < hit.sum()
    assert 4 * differ >= hit.sum()


def test_tables_without_a_v_axis_and_the_other_volumes():
    """the 1 x 1 and 3 x 1 tables (nv = 1: no second row to differ from) and the
    BAKE and f16 frames: hit pixels of several colours, and not the frame of another
    table of the same pair"""
    for pair, table, other in (("13-2", "one", "t255x4"), ("10-11", "t3x1", "t1x5")):
        for dims, nb, dtype in ((DIMS, 8, "f32"), (DIMS, 8, "f16"), (BAKE, 4, "f32")):
            rgba8, _, n, _ = reference(pair, table, dims, nb, dtype, "C1", W, H)
            base = reference(pair, other, dims, nb, dtype, "C1", W, H)
            hit = n >= 0
            assert hit.sum() > (100 if dims == DIMS else 20), (pair, table, dims)
            assert np.unique(rgba8[hit]).size > 1
            assert (rgba8 != base[0]).sum() > hit.sum() // 2, (pair, table, dims, dtype)
