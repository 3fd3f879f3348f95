"""The value ranges and histograms of baked planes without a
GPU: the numpy restatement (tests/ref_histogram.py) in its array form against its
scalar loop, the totals, the special values, a census over the five mutants on the
shapes of the GPU tests, and the host side of the C ABI: header, exports and every
refusal the library makes before it touches a device."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import ref_histogram as rh

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 32  # VR_QUERY_GRADIENT

# (nx, ny, nz), the windows and the bins of the census: uniform values in [0, 1) leave
# the u window on both sides ((s - 0.1) * 1.3 spans -0.13 .. 1.17) and the v window above
CENSUS_SHAPES = ((16, 2, 1), (31, 9, 5), (37, 20, 11))
WU, WV = (0.1, 1.3), (-0.2, 0.9)
NU, NV = 16, 8


@functools.lru_cache(maxsize=None)
def uniform_planes(dims):
    """two seeded planes (nz, ny, nx) of uniform values in [0, 1), read-only"""
    nx, ny, nz = dims
    rng = np.random.default_rng(2710 + nx)
    out = tuple(rng.random((nz, ny, nx)).astype(np.float32) for _ in range(2))
    for a in out:
        a.setflags(write=False)
    return out


def boxes_of(dims):
    nx, ny, nz = dims
    yield None
    yield (0, nx, 0, ny, 0, nz)
    yield (nx // 2, nx, 0, max(ny // 2, 1), nz - 1, nz)
    yield (nx - 1, nx, ny - 1, ny, 0, 1)


# ---- the array form against the scalar loop ----

@pytest.mark.parametrize("dims", CENSUS_SHAPES + ((1, 1, 1), (15, 1, 3)),
                         ids=lambda d: "x".join(map(str, d)))
def test_the_array_form_is_the_scalar_loop(dims):
    pu, pv = uniform_planes(dims)
    for box in boxes_of(dims):
        for nu, nv in ((1, 1), (9, 1), (NU, NV)):
            a = rh.histogram(pu, nu, WU, pv, nv, WV, box)
            b = rh.histogram_scalar(pu, nu, WU, pv, nv, WV, box)
            assert a.dtype == np.uint64 and a.shape == (nv, nu)
            assert np.array_equal(a, b), (dims, box, nu, nv)
        a = rh.histogram(pu, 7, WU, box=box)
        assert np.array_equal(a, rh.histogram_scalar(pu, 7, WU, box=box))
        assert np.array_equal(a[0], rh.histogram(pu, 7, WU, pv, 3, WV, box).sum(axis=0))
        ra, rb = rh.plane_range(pu, box), rh.plane_range_scalar(pu, box)
        assert [f32(v).view(np.uint32) for v in ra[:2]] == [f32(v).view(np.uint32) for v in rb[:2]]
        assert ra[2] == rb[2] == 0


@pytest.mark.parametrize("dims", CENSUS_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_counts_sum_to_the_voxels_of_the_box(dims):
    nx, ny, nz = dims
    pu, pv = uniform_planes(dims)
    for box in boxes_of(dims):
        x0, x1, y0, y1, z0, z1 = box or (0, nx, 0, ny, 0, nz)
        want = (x1 - x0) * (y1 - y0) * (z1 - z0)
        assert int(rh.histogram(pu, NU, WU, pv, NV, WV, box).sum()) == want
        assert int(rh.histogram(pu, 256, WU, box=box).sum()) == want


# ---- the specials ----

def _plane(values):
    return np.array(values, np.float32).reshape(1, 1, -1)


def test_the_special_values():
    inf, nan = f32(np.inf), f32(np.nan)
    off, scale, n = f32(0.25), f32(2.0), 8
    end = f32(off + f32(1) / scale)  # x = 1 exactly: the window's upper end
    s = _plane([nan, inf, -inf, 0.0, -0.0, off, end, np.nextafter(end, f32(0)), 0.5, 1e30, -1e30])
    assert list(rh.bin_of(s, off, scale, n).ravel()) == [0, n - 1, 0, 0, 0, 0, n - 1, n - 1, 4,
                                                         n - 1, 0]
    assert np.array_equal(rh.histogram(s, n, (off, scale)),
                          rh.histogram_scalar(s, n, (off, scale)))
    # a negative scale turns the axis round; a scale of 0 puts everything in bin 0, an
    # infinity included (inf * 0 is NaN)
    assert list(rh.bin_of(s, off, -scale, n).ravel()) == [0, 0, n - 1, 4, 4, 0, 0, 0, 0, 0, n - 1]
    assert not rh.bin_of(s, off, f32(0), n).any()
    for w in ((off, -scale), (off, f32(0))):
        assert np.array_equal(rh.histogram(s, n, w), rh.histogram_scalar(s, n, w))
    # +0 and -0 with offset 0 share bin 0; one bin holds everything
    assert list(rh.bin_of(_plane([0.0, -0.0]), 0.0, 1.0, 4).ravel()) == [0, 0]
    one = rh.histogram(s, 1, (off, scale), s, 1, (0.0, 1.0))
    assert one.shape == (1, 1) and int(one[0, 0]) == s.size
    # a bin is the cell [i / n, (i + 1) / n): its lower edge belongs to it, and its centre
    # is where the table's filter has weight 1 on entry i
    edges = _plane([i / 8 for i in range(8)])
    assert list(rh.bin_of(edges, 0.0, 1.0, 8).ravel()) == list(range(8))
    centres = _plane([(i + 0.5) / 8 for i in range(8)])
    assert list(rh.bin_of(centres, 0.0, 1.0, 8).ravel()) == list(range(8))
    assert list(rh.bin_of(centres, 0.0, 1.0, 8, "nearest").ravel()) == list(range(8))
    assert list(rh.bin_of(edges, 0.0, 1.0, 8, "nearest").ravel()) == [0, 0, 1, 2, 3, 4, 5, 6]


def test_the_range_orders_by_bit_pattern():
    nan = f32(np.nan)
    lo, hi, n = rh.plane_range(_plane([0.0, -0.0, nan]))
    assert (f32(lo).view(np.uint32), f32(hi).view(np.uint32), n) == (0x80000000, 0, 1)
    lo, hi, n = rh.plane_range(_plane([-0.0, 0.0]))
    assert (f32(lo).view(np.uint32), f32(hi).view(np.uint32), n) == (0x80000000, 0, 0)
    lo, hi, n = rh.plane_range(_plane([nan, 3.0, -np.inf, np.inf, -2.0, nan]))
    assert (lo, hi, n) == (-np.inf, np.inf, 2)
    neg = np.array([0xFFC00000], np.uint32).view(np.float32)  # a NaN with its sign set
    lo, hi, n = rh.plane_range(_plane([nan, neg[0]]))
    assert np.isnan(lo) and np.isnan(hi) and n == 2
    assert f32(lo).view(np.uint32) == f32(hi).view(np.uint32) == 0x7FC00000
    assert rh.plane_range_scalar(_plane([nan, neg[0]]))[2] == 2
    lo, hi, n = rh.plane_range(_plane([1.5, -1.5, 1e-45, -1e-45]))
    assert (lo, hi, n) == (f32(-1.5), f32(1.5), 0)
    # the window of a range, and of a constant plane
    assert rh.window(_plane([0.25, 0.75])) == (0.25, 2.0)
    assert rh.window(_plane([0.5, 0.5])) == (0.5, 1.0)


# ---- census over mutants ----

@pytest.mark.parametrize("dims", CENSUS_SHAPES, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("mutant", rh.MUTANTS)
def test_every_mutant_shows(mutant, dims):
    pu, pv = uniform_planes(dims)
    right = rh.histogram(pu, NU, WU, pv, NV, WV)
    wrong = rh.histogram(pu, NU, WU, pv, NV, WV, mutant=mutant)
    assert not np.array_equal(right, wrong), (mutant, dims)
    assert int(right.sum()) == pu.size
    if mutant in ("aprons", "empty_slots"):
        assert int(wrong.sum()) > pu.size
    if mutant == "dropped":
        # the window leaves values outside, and the reference keeps them in its edge bins
        xu, xv = rh.coordinate(pu, *WU), rh.coordinate(pv, *WV)
        out = (xu < 0) | (xu > 1) | (xv < 0) | (xv > 1)
        assert out.any() and int(wrong.sum()) == pu.size - int(out.sum())
        assert int(right[:, 0].sum()) >= int((xu < 0).sum())
        assert int(right[:, -1].sum()) >= int((xu > 1).sum())
        assert int(right[-1].sum()) >= int((xv > 1).sum())
        assert int((xu < 0).sum()) + int((xu > 1).sum()) + int((xv > 1).sum()) >= int(out.sum()) > 0


def test_the_box_mutants_show_in_a_box():
    """aprons and empty slots inside a box as well, which the GPU box tests rely on"""
    pu, pv = uniform_planes((37, 20, 11))
    for box in ((15, 31, 3, 9, 2, 5), (30, 37, 0, 20, 0, 11)):
        right = rh.histogram(pu, NU, WU, pv, NV, WV, box)
        assert not np.array_equal(right, rh.histogram(pu, NU, WU, pv, NV, WV, box, "aprons"))
    box = (30, 37, 0, 20, 0, 11)
    assert not np.array_equal(rh.histogram(pu, NU, WU, pv, NV, WV, box),
                              rh.histogram(pu, NU, WU, pv, NV, WV, box, "empty_slots"))


# ---- header, exports and refusals, no device call ----

def test_header_and_exports(pkg):
    src = open(os.path.join(ROOT, "include", "vr.h")).read()
    assert re.search(r"#define\s+VR_HIST_MAX\s+16384\b", src)
    for name in ("vr_plane_range", "vr_plane_histogram", "vr_plane_kernel_ms"):
        assert re.search(rf"\bint {name}\(", src), name
        assert name in pkg._lib.EXPORTS and hasattr(pkg._lib.load(), name), name
    for name in ("HIST_MAX", "plane_range", "plane_window", "plane_histogram", "plane_kernel_ms"):
        assert name in pkg.api.__all__ and hasattr(pkg, name), name
    assert pkg.HIST_MAX == pkg._lib.VR_HIST_MAX == 16384


PLANES = (1, 2, 3, 4, 5, 6, 10, 11, 12, 13)


def _hist(L, mu, nu, mv=0, nv=1, wu=(0.0, 1.0), wv=(0.0, 1.0), box=None, counts=True):
    buf = (ctypes.c_uint64 * max(1, min(nu * nv, 16384) if nu > 0 and nv > 0 else 1))()
    b = (ctypes.c_int * 6)(*box) if box is not None else None
    return L.vr_plane_histogram(mu, wu[0], wu[1], nu, mv, wv[0], wv[1], nv,
                                ctypes.addressof(b) if b else None,
                                ctypes.addressof(buf) if counts else None)


def _range(L, m, box=None):
    b = (ctypes.c_int * 6)(*box) if box is not None else None
    out = (ctypes.c_float * 2)()
    n = ctypes.c_uint64()
    return L.vr_plane_range(m, ctypes.addressof(b) if b else None, ctypes.addressof(out),
                            ctypes.addressof(out) + 4, ctypes.addressof(n))


def test_refusals_without_gpu(pkg):
    """everything the library refuses before it touches a device, with nothing resident"""
    L, lib = pkg._lib.load(), pkg._lib
    pkg.freeCudaBuffers()
    L.vr_clear_error()
    inf, nan = float("inf"), float("nan")
    # methods that name no plane
    for m in (0, 7, 8, 9, 14, 31, 32, G + 7, G + 14, -1):
        assert _range(L, m) == lib.VR_ERR_ARG, m
        assert _hist(L, m, 8) == lib.VR_ERR_ARG, m
        if m != 0:
            assert _hist(L, 1, 8, m, 4) == lib.VR_ERR_ARG, m
    # bin counts
    for nu, nv, mv in ((0, 1, 0), (-1, 1, 0), (8, 0, 2), (8, -3, 2), (16385, 1, 0), (129, 128, 2),
                       (16384, 2, 2), (1 << 30, 1 << 30, 2), (8, 2, 0), (8, 0, 0)):
        assert _hist(L, 1, nu, mv, nv) == lib.VR_ERR_ARG, (nu, nv, mv)
    # windows
    for w in ((inf, 1.0), (0.0, inf), (nan, 1.0), (0.0, nan), (0.0, -inf)):
        assert _hist(L, 1, 8, wu=w) == lib.VR_ERR_ARG, w
        assert _hist(L, 1, 8, 2, 8, wv=w) == lib.VR_ERR_ARG, w
    # boxes that are empty or start below 0, whatever the grid
    for box in ((0, 0, 0, 1, 0, 1), (2, 1, 0, 1, 0, 1), (0, 1, 3, 3, 0, 1), (0, 1, 0, 1, 5, 4),
                (-1, 1, 0, 1, 0, 1), (0, 1, 0, 1, -2, 1)):
        assert _hist(L, 1, 8, box=box) == lib.VR_ERR_ARG, box
        assert _range(L, 1, box) == lib.VR_ERR_ARG, box
    assert _hist(L, 1, 8, counts=False) == lib.VR_ERR_ARG
    assert "counts" in L.vr_last_error().decode()
    # planes of different volumes, before either has to be there
    for mu, mv in ((1, 4), (5, 2), (G + 1, 6), (13, G + 4), (4, 11)):
        assert _hist(L, mu, 8, mv, 4) == lib.VR_ERR_UNSUPPORTED, (mu, mv)
    # nothing resident: a state error that names the bake
    for m, call in ((1, "vr_bake_stats"), (5, "vr_bake_stats"), (10, "vr_bake_weighted"),
                    (11, "vr_bake_quantile"), (12, "vr_bake_distance"), (13, "vr_bake_crossing"),
                    (G + 2, "vr_bake_gradient(2)"), (G + 13, "vr_bake_gradient(13)")):
        assert _range(L, m) == lib.VR_ERR_STATE
        assert call in L.vr_last_error().decode(), L.vr_last_error()
        assert _hist(L, m, 8) == lib.VR_ERR_STATE
        assert call in L.vr_last_error().decode(), L.vr_last_error()
        assert _hist(L, m, 8, m, 4) == lib.VR_ERR_STATE
    # the wrappers raise what the library says
    with pytest.raises(pkg.VRError) as e:
        pkg.plane_range(7)
    assert e.value.status == lib.VR_ERR_ARG
    with pytest.raises(pkg.VRError) as e:
        pkg.plane_histogram(1, 8, window_u=(0.0, 1.0))
    assert e.value.status == lib.VR_ERR_STATE
    with pytest.raises(pkg.VRError) as e:
        pkg.plane_histogram(1, 200, (0.0, 1.0), 2, 200, (0.0, 1.0))
    assert e.value.status == lib.VR_ERR_ARG
    with pytest.raises(pkg.VRError) as e:
        pkg.plane_histogram(1, 8, (0.0, 1.0), nv=2)
    assert e.value.status == lib.VR_ERR_ARG
    with pytest.raises(pkg.VRError) as e:
        pkg.plane_window(1)  # the default window asks for the range first
    assert e.value.status == lib.VR_ERR_STATE
    with pytest.raises(ValueError):
        pkg.plane_range(1, box=(0, 1, 0, 1))
    assert pkg.plane_kernel_ms() >= 0.0
    L.vr_clear_error()
