"""Seeded random parity sweep of the plane kernels that march no ray, and the walk of
whole volumes:

  k_bake_grad (gradient-magnitude planes, vr_gradient.hip):
  random_cases.grad_case, 24 bakes at the sizes where its tiles (60 voxels of x plus an
  apron, 16 rows, 64 slices read ahead four at a time) begin and end, from record (fp32,
  f16) and codec volumes and every source method, a quarter of them over planes of
  wide dynamic range, both zeros and denormals, three with infinities and NaNs;
  k_plane_range and k_plane_hist (vr_histogram.hip, section 27): random_cases.stat_case,
  48 calls over every kind of box, every number of LDS copies in the 1-D and the 2-D
  form, six kinds of window, planes and gradient planes on either axis, a quarter with
  special values injected and every slot that is no voxel's home poisoned;
  and the same two kernels over volumes of more than 2 x (2 x CUs) rounds of 128 lines,
  where a workgroup walks several rounds: the digit-by-digit stride with its carries,
  all three stages of the register pipeline, counters that accumulate in LDS, the tail.

Every comparison is exact.  A baked gradient plane is the whole buffer -- homes, aprons,
empty slots, tail padding -- and the maximum, bit for bit against tests/ref_gradient.py
over the source plane the device holds; where the reference magnitude is NaN the device's
must be a NaN (the host's and the GPU's default NaN differ in their sign) and the
maximum is then NaN.  Ranges are bit patterns and the NaN count, histograms every count,
against tests/ref_histogram.py over the un-bricked planes the device holds.
tests/test_random_planes.py checks on the CPU that the cases deal what they are there
for and that each mutant of the references would be noticed.  A failure message carries
the seed and the whole case.

Seconds per case on one MI355X, reference included (the CASE lines of a run with -s):
grad 0.02 mean / 0.14 at most, stat 0.01 / 0.08; the walks of whole volumes take 1.0 s
(100 x 37 x 1400) and 1.2 s (3750 x 599 x 3); the file takes 6 s.
"""
import functools
import time

import numpy as np
import pytest

import random_cases as rc
import ref_gradient
from test_gpu_f16 import d2h
from test_gpu_gradient import bricked
from test_gpu_histogram import (HIST0, HIST1, bits, check_hist, check_range, device_plane, h2d,
                                home_index, plane_ptr)
from test_gpu_random_queries import report
from test_gpu_random_transfer import bake_planes
from test_random_planes import (G, box_voxels, inject, refused, source_methods, stat_expected,
                                stat_windows)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    def clear():
        pkg.set_light(None)
        pkg.set_projection(None)
        pkg.set_transfer_function(None)
        pkg.set_transfer_function_2d(None)
        pkg.set_crossing_weights(None)
        pkg.set_query_target(None)
        pkg.set_quantile(None)
        pkg.set_bin_weights(None)
        pkg.set_stream(None)
        pkg.clear_tuning()
    clear()
    pkg.freeCudaBuffers()
    yield
    clear()
    pkg.freeCudaBuffers()


def bake_sources(pkg, orc, case, what):
    """the volume of a grad or stat case resident with the planes of its source methods"""
    src = source_methods(case)
    bake_planes(pkg, orc, dict(case, u=src[0], v=src[1] if len(src) > 1 else None), what)


# ---- k_bake_grad ----

@pytest.mark.parametrize("seed", range(rc.PLANE_SWEEPS["grad"][1]))
def test_random_gradient_case(pkg, orc, gpu, seed):
    t0 = time.perf_counter()
    case = rc.grad_case(seed)
    what = f"seed {seed}: {case}"
    u, dims, fill = case["u"], case["dims"], case["fill"]
    bake_sources(pkg, orc, case, what)
    ptr, n = plane_ptr(pkg, u)
    home, floats = home_index(dims)
    assert ptr and n == floats, what
    if fill is not None:  # the whole layout anew: homes and their apron copies
        h2d(ptr, bricked(rc.make_wide(fill, dims[::-1])))
    flat = d2h(ptr, n, np.float32)
    s = flat[home]
    if fill is not None:
        assert np.array_equal(s.view(np.uint32), rc.make_wide(fill, dims[::-1]).view(np.uint32))
    assert pkg.gradient_info(u) == (None, 0, 0.0), what
    pkg.bake_gradient(u)
    assert pkg.last_kernel().startswith("k_bake_grad"), pkg.last_kernel()
    gptr, gn, mx = pkg.gradient_info(u)
    with np.errstate(all="ignore"):
        mag, _ = ref_gradient.gradient_plane(s)
    want = np.concatenate([bricked(mag), np.zeros(4, np.float32)])
    assert gptr and gn == n == want.size - 4, what
    got = d2h(gptr, gn + 4, np.float32)
    nan = np.isnan(want)
    finite_case = fill is None or not fill["nonfinite"]
    if finite_case:
        assert not nan.any(), what
    else:
        assert nan.any() and (~nan & (want != 0)).any(), what
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:8], got[bad][:4],
                           want[bad][:4])
    assert np.isnan(got[nan]).all(), (what, int((~np.isnan(got[nan])).sum()))
    if nan.any():  # the unsigned maximum of the bit patterns: any NaN is above +inf
        assert np.isnan(mx), (what, mx)
    else:
        want_max = ref_gradient.bits_max(mag)
        assert bits(mx) == bits(want_max), (what, mx, want_max)
        lo, hi, nn = pkg.plane_range(G + u)
        assert bits(hi) == bits(mx) and nn == 0, (what, hi, mx, nn)
    # the source is untouched
    assert np.array_equal(d2h(ptr, n, np.float32).view(np.uint32), flat.view(np.uint32)), what
    report(case, "k_bake_grad", t0)


# ---- k_plane_range and k_plane_hist ----

@pytest.mark.parametrize("seed", range(rc.PLANE_SWEEPS["stat"][1]))
def test_random_range_and_histogram_case(pkg, orc, gpu, seed):
    t0 = time.perf_counter()
    case = rc.stat_case(seed)
    what = f"seed {seed}: {case}"
    u, v, dims, box = case["u"], case["v"], case["dims"], case["box"]
    methods = (u,) if v is None or v == u else (u, v)
    bake_sources(pkg, orc, case, what)
    for mth in methods:
        if mth > G:
            pkg.bake_gradient(mth - G)
    if case["inject"] is not None:
        # special values in plane u, and every float that is no voxel's home -- aprons,
        # empty slots -- set to a value that would count if it were read
        ptr, n = plane_ptr(pkg, u)
        home, floats = home_index(dims)
        poison = np.full(floats, 7.0, np.float32)
        poison[home.ravel()] = inject(case["inject"], device_plane(pkg, u, dims)).ravel()
        h2d(ptr, poison)
    planes = {mth: device_plane(pkg, mth, dims) for mth in methods}
    for mth in methods:
        check_range(pkg, mth, planes[mth], box, what=what)
    (wu, wv), ref_windows = stat_windows(case, planes)
    if refused(ref_windows):  # the range of a plane that holds an infinity is no window
        with pytest.raises(pkg.VRError) as e:
            pkg.plane_histogram(u, case["nu"], wu, v, case["nv"], wv, box)
        assert e.value.status == pkg._lib.VR_ERR_ARG and case["inject"] is not None, what
        report(case, pkg.last_kernel(), t0)
        return
    want = stat_expected(case, planes)
    got = pkg.plane_histogram(u, case["nu"], wu, v, case["nv"], wv, box)
    kernel = pkg.last_kernel()
    assert kernel == (HIST0 if v is None else HIST1), (what, kernel)
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.shape)
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4],
                           want[bad][:4])
    assert int(got.sum()) == box_voxels(case), what
    report(case, kernel, t0)


# ---- volumes a workgroup walks in several rounds ----

# (100, 37, 1400): 7 bricks x 19 y pairs x 1400 slices = 186 200 lines, 1455 rounds of 128;
# on 256 CUs the stride of 65 536 lines has the digits da = 2, db = 14, dc = 492: carries
# into both higher digits.  (3750, 599, 3): 250 bricks x 300 pairs = 75 000 lines a slice,
# more than the stride, so dc = 0 and the slice advances by carry alone, as in a 1024^3
# volume.  The boxes start at neither brick 0, pair 0 nor slice 0.
WALKS = {(100, 37, 1400): (16, 95, 3, 36, 5, 1399), (3750, 599, 3): (16, 3750, 3, 599, 1, 3)}
LINES = 128


def lines_of(dims, box=None):
    nx, ny, nz = dims
    x0, x1, y0, y1, z0, z1 = box or (0, nx, 0, ny, 0, nz)
    return ((x1 - 1) // 15 - x0 // 15 + 1) * ((y1 - 1) // 2 - y0 // 2 + 1) * (z1 - z0)


def test_lines_of():
    assert lines_of((100, 37, 1400)) == 186200 and lines_of((3750, 599, 3)) == 225000
    assert lines_of((100, 37, 1400), WALKS[(100, 37, 1400)]) == 142188
    assert lines_of((70, 19, 67)) == 3350


@functools.lru_cache(maxsize=None)
def _homes(dims):
    return home_index(dims)


def put(pkg, method, dims, p):
    """the plane p (nz, ny, nx) into the home slots of the resident plane of `method`;
    every other slot is set to 7.0, which would count if it were read"""
    ptr, n = plane_ptr(pkg, method)
    home, floats = _homes(dims)
    assert ptr and n == floats
    flat = np.full(floats, 7.0, np.float32)
    flat[home.ravel()] = p.ravel()
    h2d(ptr, flat)


@pytest.mark.parametrize("dims", list(WALKS), ids=lambda d: "x".join(map(str, d)))
def test_a_workgroup_walks_several_rounds(pkg, gpu, dims):
    import torch
    t0 = time.perf_counter()
    nx, ny, nz = dims
    box = WALKS[dims]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = 2 * cus
    for b in (None, box):  # every workgroup walks at least two rounds, most of them more
        rounds = (lines_of(dims, b) + LINES - 1) // LINES
        assert rounds >= 2 * grid if b is None else rounds > grid, (dims, b, rounds, cus)
    pkg.synthesize(dims, 1)
    pkg.bake_stats()
    rng = np.random.default_rng(2800 + nx)
    p1 = rng.random((nz, ny, nx), dtype=np.float32)
    p2 = (rng.standard_normal((nz, ny, nx), dtype=np.float32) * np.float32(0.25)
          + p1 * np.float32(0.5)).astype(np.float32)
    p1.ravel()[rng.choice(p1.size, 5, replace=False)] = np.nan
    p1[nz - 1, ny - 1, nx - 1] = np.nan   # the last line of the walk
    p1[0, 0, 0] = -3.0                    # and the extremes in its first and in a middle one
    p1[nz // 2, ny // 2, nx // 2] = 5.0
    planes = {1: p1, 2: p2}
    put(pkg, 1, dims, p1)
    put(pkg, 2, dims, p2)
    what = f"{dims} random planes"
    assert check_range(pkg, 1, p1, what=what) == (np.float32(-3.0), np.float32(5.0), 6)
    check_range(pkg, 2, p2, what=what)
    check_hist(pkg, planes, 1, 256, (0.0, 1.0), what=what)
    check_hist(pkg, planes, 1, 64, (0.0, 1.0), 2, 64, (-0.5, 0.5), what=what)
    check_hist(pkg, planes, 1, 128, None, 2, 128, None, what=what)
    what = f"{dims} box {box}"
    check_range(pkg, 1, p1, box, what=what)
    check_range(pkg, 2, p2, box, what=what)
    check_hist(pkg, planes, 2, 256, (-0.5, 0.5), box=box, what=what)
    check_hist(pkg, planes, 1, 64, (0.0, 1.0), 2, 64, (-0.5, 0.5), box, what=what)
    # a constant plane: the wave's pre-count, a workgroup's counters over all its rounds
    c1 = np.full((nz, ny, nx), 0.375, np.float32)
    planes = {1: c1, 2: p2}
    put(pkg, 1, dims, c1)
    what = f"{dims} constant plane"
    assert check_range(pkg, 1, c1, what=what) == (np.float32(0.375), np.float32(0.375), 0)
    h = check_hist(pkg, planes, 1, 256, (0.0, 1.0), what=what)
    assert int(h[0, 96]) == c1.size
    h = check_hist(pkg, planes, 1, 128, (0.0, 1.0), 1, 128, (0.0, 1.0), what=what)
    assert int(h[48, 48]) == c1.size
    check_hist(pkg, planes, 1, 64, (0.0, 1.0), 2, 64, (-0.5, 0.5), what=what)
    # constant but for one voxel of the last slice: the tail round
    c1[nz - 1, ny - 1, nx - 2] = 0.875
    put(pkg, 1, dims, c1)
    what = f"{dims} nearly constant plane"
    assert check_range(pkg, 1, c1, what=what) == (np.float32(0.375), np.float32(0.875), 0)
    check_range(pkg, 1, c1, box, what=what)
    h = check_hist(pkg, planes, 1, 256, (0.0, 1.0), what=what)
    assert int(h[0, 224]) == 1 and int(h[0, 96]) == c1.size - 1
    h = check_hist(pkg, planes, 1, 64, (0.0, 1.0), 1, 64, (0.0, 1.0), what=what)
    assert int(h[56, 56]) == 1 and int(h[24, 24]) == c1.size - 1
    print(f"\nWALK {dims} rounds {(lines_of(dims) + LINES - 1) // LINES} CUs {cus} "
          f"seconds {time.perf_counter() - t0:.2f}")
