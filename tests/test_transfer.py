"""The user-defined transfer function without a GPU: known
answers of the numpy classifier, the classifier with the reference's nine entries
against the built-in one bit for bit (samples and whole frames), the host state of
the C ABI (vr_set_transfer_function makes no device call), and the reference frames
the GPU tests compare against."""
import ctypes
import functools

import numpy as np
import pytest

import ref_crossing
import ref_numpy
import ref_transfer
from test_crossing import BAKE, DIMS, H, W, camera, cdf

f32 = np.float32
T = ref_transfer.transfer_table

SPECIALS = f32([-np.inf, -1.0, -0.0, 0.0, 1.0, 2.0, np.inf, np.nan, 2.0 ** -140, -2.0 ** -140])


# ---- the tables of the tests (read-only, shared with tests/test_gpu_transfer.py) ----

def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


RAMP2 = _ro([(0, 0, 1, 0), (1, 0, 0, 1)])                      # an opacity ramp, blue to red
RAND256 = _ro(np.random.default_rng(1401).random((256, 4)))    # every entry, every channel
ONE = _ro([(0.25, 0.5, 0.75, 0.5)])                            # n = 1: one thread stages
N255 = _ro(np.random.default_rng(1402).random((255, 4)))       # n = 255: one thread stages nothing
TABLES = {"ramp2": RAMP2, "rand256": RAND256, "one": ONE, "n255": N255}
BLENDS = {"combine": ref_crossing.combine, "trilinear": ref_crossing.trilinear}


# ---- known answers of transfer_table ----

def test_one_entry_is_constant():
    x = np.concatenate([np.linspace(-1, 2, 301, dtype=np.float32), SPECIALS])
    got = T(x, ONE)
    assert got.dtype == np.float32 and got.shape == (x.size, 4)
    assert np.all(got == ONE[0])  # (1 - a) * v + a * v with a a multiple of 2^-8: exact here


def test_two_entries():
    """entry i is centred at (i + 1/2) / n: x = 0.25 and 0.75 hit the entries, x = 0.5
    is half way, and outside [0.25, 0.75] the clamped indices repeat an entry"""
    assert np.array_equal(T(f32(0.25), RAMP2), RAMP2[0])
    assert np.array_equal(T(f32(0.75), RAMP2), RAMP2[1])
    assert np.array_equal(T(f32(0.5), RAMP2), f32([0.5, 0, 0.5, 0.5]))
    assert np.array_equal(T(f32(0.375), RAMP2), f32([0.25, 0, 0.75, 0.25]))
    for x in (0.0, 0.1, 0.2):
        assert np.array_equal(T(f32(x), RAMP2), RAMP2[0]), x
    for x in (0.8, 0.9, 1.0):
        assert np.array_equal(T(f32(x), RAMP2), RAMP2[1]), x


def test_the_weight_is_quantised_to_one_256th():
    """x = 0.25 + d / 2 has the exact weight d; the table sees rint(256 d) / 256"""
    tab = f32([(0, 0, 0, 0), (256, 256, 256, 256)])
    for d, q in ((1 / 256, 1), (1 / 512 + 1 / 4096, 1), (1 / 1024, 0), (100.3 / 256, 100),
                 (3 / 512, 2), (1 / 512, 0)):  # the last two: ties go to even
        got = T(f32(0.25 + d / 2), tab)
        assert np.all(got == f32(q)), (d, q, got)


def test_clamping_is_transfer_s():
    """x < 0 is x = 0, x > 1 is x = 1, -inf / +inf with them, NaN is 0"""
    lo, hi = T(f32(0), RAND256), T(f32(1), RAND256)
    assert np.array_equal(lo, RAND256[0]) and np.array_equal(hi, RAND256[255])
    for x in (-1e-30, -0.5, -1e30, -np.inf, np.nan):
        assert np.array_equal(T(f32(x), RAND256), lo), x
    for x in (1.0000001, 1.5, 1e30, np.inf):
        assert np.array_equal(T(f32(x), RAND256), hi), x
    assert np.array_equal(ref_numpy.transfer(f32(np.nan)), ref_numpy.transfer(f32(0)))
    # nothing in the table is clamped
    assert np.array_equal(T(f32(0.5), f32([(-3, 7, 1e30, -0.0)])), f32([-3, 7, 1e30, 0]))


# ---- with the reference's nine entries: the built-in classifier ----

def test_reference_table_is_the_built_in_one(pkg):
    assert pkg.REFERENCE_TF.shape == (9, 4) and pkg.REFERENCE_TF.dtype == np.float32
    assert np.array_equal(pkg.REFERENCE_TF, ref_numpy.TF)
    assert not pkg.REFERENCE_TF[0].any() and not pkg.REFERENCE_TF[8].any()  # 0 and 1 vanish
    k = np.arange(-16384, 81921, dtype=np.int64)  # every k / 65536 in [-0.25, 1.25]
    x = np.concatenate([(k.astype(np.float64) / 65536.0).astype(np.float32), SPECIALS])
    assert x[0] == f32(-0.25) and x[k.size - 1] == f32(1.25)
    with np.errstate(all="ignore"):
        want = ref_numpy.transfer(x).astype(np.float32)
    got = T(x, pkg.REFERENCE_TF)
    assert got.tobytes() == want.tobytes()
    assert np.unique(got, axis=0).shape[0] > 1000


@pytest.mark.parametrize("blend", sorted(BLENDS))
def test_frames_with_the_reference_table_are_the_built_in_frames(pkg, blend):
    F, m = cdf(DIMS, 8, "f32"), camera("C1")
    want = ref_crossing.render_plane(F, W, H, m, blend=BLENDS[blend])
    got = ref_transfer.render_plane(F, W, H, m, pkg.REFERENCE_TF, blend=BLENDS[blend])
    assert (want[2] >= 0).sum() > 500
    for g, r in zip(got, want):
        assert g.dtype == r.dtype and np.array_equal(g, r)
    assert ref_crossing.transfer is ref_numpy.transfer  # the binding is undone


# ---- host state of the C ABI ----

def _state(pkg):
    t = pkg.transfer_function()
    return None if t is None else t.tobytes()


def test_transfer_state_without_gpu(pkg):
    L, lib = pkg._lib.load(), pkg._lib
    assert lib.VR_TF_MAX == pkg.TF_MAX == 256
    pkg.freeCudaBuffers()
    pkg.set_transfer_function(None)
    L.vr_clear_error()
    assert pkg.transfer_function() is None
    n = ctypes.c_int(-1)
    assert L.vr_transfer_function(None, ctypes.addressof(n)) == lib.VR_OK and n.value == 0
    assert L.vr_transfer_function(None, None) == lib.VR_OK
    # set, read back, replace
    for tab in (ONE, RAMP2, pkg.REFERENCE_TF, N255, RAND256, -RAND256 * f32(3)):
        pkg.set_transfer_function(tab)
        got = pkg.transfer_function()
        assert got.dtype == np.float32 and got.shape == tab.shape and np.array_equal(got, tab)
        assert L.vr_transfer_function(None, ctypes.addressof(n)) == lib.VR_OK
        assert n.value == tab.shape[0]
    pkg.set_transfer_function([[0, 0, 0, 0], [1, 1, 1, 1]])  # any array-like
    with pytest.raises(ValueError):
        pkg.set_transfer_function(np.zeros((3, 3), np.float32))
    # errors leave the state as it was
    pkg.set_transfer_function(RAMP2)
    keep = _state(pkg)
    big = np.zeros((300, 4), np.float32)
    for n_bad in (0, -1, 257, 300, 1 << 20):
        assert L.vr_set_transfer_function(big.ctypes.data, n_bad) == lib.VR_ERR_ARG
        assert _state(pkg) == keep
    for bad in (np.nan, np.inf, -np.inf):
        for where in ((0, 0), (1, 3), (8, 2)):
            t = pkg.REFERENCE_TF.copy()
            t[where] = bad
            with pytest.raises(pkg.VRError) as e:
                pkg.set_transfer_function(t)
            assert e.value.status == lib.VR_ERR_ARG and "finite" in str(e.value)
            assert _state(pkg) == keep
    # the table is the caller's: it outlives freeCudaBuffers, the other queries'
    # state and their planes' releases; nothing so far has made a device call
    pkg.freeCudaBuffers()
    pkg.release_stats()
    pkg.release_crossing()
    pkg.set_bin_weights([1.0, 2.0])
    pkg.set_bin_weights(None)
    assert _state(pkg) == keep
    L.vr_clear_error()
    pkg.set_transfer_function(RAND256)
    assert L.vr_last_status() == lib.VR_OK and L.vr_last_error() == b""
    # only a NULL call clears it (n is not read)
    assert L.vr_set_transfer_function(None, 77) == lib.VR_OK
    assert pkg.transfer_function() is None


def test_refusals_come_before_any_device_work(pkg):
    """with a table set, what has no plane march is refused outright -- the counts
    before they look at their descriptor"""
    L, lib = pkg._lib.load(), pkg._lib
    pkg.freeCudaBuffers()
    pkg.set_transfer_function(RAMP2)
    try:
        d = pkg.make_desc(0x1000, W, H, camera("C0"), query_method=1, volume_size=(4, 4, 4))
        for call in (L.vr_count_footprint, L.vr_footprint_bytes, L.vr_gmm_count_footprint):
            assert call(ctypes.byref(d)) == lib.VR_ERR_UNSUPPORTED
            msg = L.vr_last_error().decode()
            assert "custom transfer function" in msg and "bake" in msg and "clear" in msg, msg
        assert L.vr_render_gmm(ctypes.byref(d), None) == lib.VR_ERR_UNSUPPORTED
        assert "custom transfer function" in L.vr_last_error().decode()
    finally:
        pkg.set_transfer_function(None)
        L.vr_clear_error()
    # cleared: the usual state error of a library without a volume
    assert L.vr_count_footprint(ctypes.byref(d)) == lib.VR_ERR_STATE
    L.vr_clear_error()


def test_exports(pkg):
    for name in ("TF_MAX", "REFERENCE_TF", "set_transfer_function", "transfer_function"):
        assert name in pkg.api.__all__ and hasattr(pkg, name), name
    for name in ("vr_set_transfer_function", "vr_transfer_function"):
        assert name in pkg._lib.EXPORTS and hasattr(pkg._lib.load(), name), name


# ---- the reference frames of the GPU tests ----

@functools.lru_cache(maxsize=None)
def reference(dims, nb, dtype, cam, w, h, table, blend):
    """the numpy frame under TABLES[table] with BLENDS[blend] over the plane of F of
    test_crossing.cdf, computed once per case and shared by the CPU and the GPU
    tests: (RGBA8, float RGBA, samples, info), arrays read-only"""
    info = {}
    ref = ref_transfer.render_plane(cdf(dims, nb, dtype), w, h, camera(cam), TABLES[table],
                                    blend=BLENDS[blend], info=info)
    for a in ref:
        a.setflags(write=False)
    return ref + (info,)


@functools.lru_cache(maxsize=None)
def rainbow(dims, nb, dtype, cam, w, h, blend):
    """the same frame under the built-in table"""
    ref = ref_crossing.render_plane(cdf(dims, nb, dtype), w, h, camera(cam), blend=BLENDS[blend])
    for a in ref:
        a.setflags(write=False)
    return ref


# (view, blend, table) -> (hit pixels, early endings) of DIMS x 8 f32 at 64 x 48
PINNED = {
    ("C0", "combine", "ramp2"): (1389, 404), ("C0", "trilinear", "ramp2"): (1389, 981),
    ("C0", "combine", "rand256"): (1389, 716), ("C0", "trilinear", "rand256"): (1389, 590),
    ("C1", "combine", "ramp2"): (1330, 425), ("C1", "trilinear", "ramp2"): (1330, 989),
    ("C1", "combine", "rand256"): (1330, 646), ("C1", "trilinear", "rand256"): (1330, 524),
}


@pytest.mark.parametrize("cam,blend,table", sorted(PINNED),
                         ids=["-".join(k) for k in sorted(PINNED)])
def test_reference_frame_is_worth_comparing(cam, blend, table):
    """by the reference alone: hit pixels of more than one colour, rays that end
    early and rays that run their full length, and another frame than the built-in
    table's on the same rays"""
    rgba8, _, n, info = reference(DIMS, 8, "f32", cam, W, H, table, blend)
    base = rainbow(DIMS, 8, "f32", cam, W, H, blend)
    hit = n >= 0
    colours = np.unique(rgba8[hit]).size
    early = int(info["early"].sum())
    differ = int((rgba8 != base[0]).sum())
    print(f"{int(hit.sum())} hit, {colours} colours, {early} early, {differ} differ")
    assert np.array_equal(hit, base[2] >= 0)
    assert (int(hit.sum()), early) == PINNED[cam, blend, table]
    assert colours > 50 and 0 < early < hit.sum()
    assert differ >= 965


def test_small_table_frames_differ_too():
    """the one-entry and 255-entry tables and the BAKE volume's frames: not the
    built-in frame either, and the one-entry frame still has pixels of several
    colours (the opacity a ray gathers depends on its length)"""
    for dims, nb, table in ((DIMS, 8, "one"), (DIMS, 8, "n255"), (BAKE, 4, "rand256")):
        for blend in sorted(BLENDS):
            rgba8, _, n, _ = reference(dims, nb, "f32", "C1", W, H, table, blend)
            base = rainbow(dims, nb, "f32", "C1", W, H, blend)
            hit = n >= 0
            assert hit.sum() > 20 and np.unique(rgba8[hit]).size > 1
            assert (rgba8 != base[0]).sum() > hit.sum() // 2, (dims, table, blend)
