"""GPU checks of the value ranges and histograms of baked planes (vr_histogram.hip,
DESIGN.md section 27).

Counts are integers and a bin is two float32 operations, a clamp and a floor, which
numpy restates bit for bit (tests/ref_histogram.py, held to its scalar loop and to five
mutants on the CPU by tests/test_histogram.py), so every comparison is exact: every
count, the total, the minimum and maximum as bit patterns and the NaN count.  The
expected figures come from the plane the device holds, un-bricked on the host.
"""
import ctypes

import numpy as np
import pytest

import ref_histogram as rh
from test_crossing import DIMS, camera, volume
from test_gpu_crossing import assert_same
from test_gpu_f16 import d2h
from test_gpu_gradient import render, upload_planes
from test_gpu_transfer2 import kernel_of
from test_gradient import PLANE_SHAPES
from test_transfer2 import CODEC, RAND32, codec_records

pytestmark = pytest.mark.gpu

f32 = np.float32
G = 32
# (16, 2, 1): x = 15 is a home and an apron; (15, 1, 3): one brick, an odd ny;
# (31, 9, 5): x = 30 in two bricks, a y pair with one row; (37, 20, 11): a partial last
# brick; (70, 19, 67): 5 bricks x 10 pairs x 67 slices = 3350 lines, 27 rounds of 128
# lines, so more than one workgroup and several slices in a workgroup's share
SHAPES = tuple(s for s in PLANE_SHAPES if s != (1, 1, 1))
HIST0, HIST1, RANGE = "k_plane_hist<B=1,M=0>", "k_plane_hist<B=1,M=1>", "k_plane_range<B=1,M=0>"


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


def bits(v):
    return int(np.float32(v).view(np.uint32))


def plane_ptr(pkg, method):
    """(device pointer, floats) of the resident plane of `method`"""
    if method > G:
        ptr, n, _ = pkg.gradient_info(method - G)
        return ptr, n
    if method <= 6:
        (raw, rn), (cod, cn) = pkg.stats_info()
        ptr, n, k = (raw, rn, method - 1) if method <= 3 else (cod, cn, method - 4)
        return ptr + 4 * n * k, n
    return {10: pkg.weighted_info, 11: pkg.quantile_info, 12: pkg.distance_info,
            13: pkg.crossing_info}[method]()


def home_index(dims):
    """the index of every voxel's home slot in the brick layout, (nz, ny, nx), and the
    layout's length in floats"""
    nx, ny, nz = dims
    sy = ((nx - 1) // 15 + 1) * 32
    sz = ((ny + 1) // 2) * sy
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return z * sz + (y // 2) * sy + (y % 2) * 16 + (x // 15) * 32 + x % 15, sz * nz


def device_plane(pkg, method, dims):
    """the resident plane of `method` un-bricked: (nz, ny, nx) float32"""
    ptr, n = plane_ptr(pkg, method)
    home, floats = home_index(dims)
    assert ptr and n == floats
    return d2h(ptr, n, np.float32)[home]


def h2d(ptr, a):
    import torch
    torch.cuda.synchronize()
    a = np.ascontiguousarray(a)
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(ptr), ctypes.c_void_p(a.ctypes.data),
                         ctypes.c_size_t(a.nbytes), 1) == 0


def inner(p):
    """a window that leaves a quarter of the plane's range outside on either side"""
    lo, hi, _ = rh.plane_range(p)
    if not hi > lo:
        return float(lo), 1.0
    return float(lo) + 0.25 * float(hi - lo), 2.0 / float(hi - lo)


def check_range(pkg, method, p, box=None, what=""):
    got = pkg.plane_range(method, box)
    assert pkg.last_kernel() == RANGE, pkg.last_kernel()
    want = rh.plane_range(p, box)
    assert (bits(got[0]), bits(got[1]), got[2]) == (bits(want[0]), bits(want[1]), want[2]), \
        (what, method, box, got, want)
    assert pkg.plane_window(method, box) == rh.window(p, box), (what, method, box)
    return got


def check_hist(pkg, planes, mu, nu, wu=None, mv=None, nv=1, wv=None, box=None, what=""):
    """one plane_histogram call against numpy; planes: method -> un-bricked plane.  A
    window of None is the library's default on both sides."""
    got = pkg.plane_histogram(mu, nu, wu, mv, nv, wv, box)
    assert pkg.last_kernel() == (HIST0 if mv is None else HIST1), pkg.last_kernel()
    pu, pv = planes[mu], planes[mv] if mv is not None else None
    wu_ = rh.window(pu, box) if wu is None else wu
    wv_ = (0.0, 1.0) if mv is None else rh.window(pv, box) if wv is None else wv
    want = rh.histogram(pu, nu, wu_, pv, nv, wv_, box)
    assert got.dtype == np.uint64 and got.shape == (nv, nu), (what, got.shape)
    bad = got != want
    assert not bad.any(), (what, mu, mv, nu, nv, box, int(bad.sum()), np.argwhere(bad)[:4].tolist(),
                           got[bad][:4], want[bad][:4])
    nx, ny, nz = pu.shape[::-1]
    x0, x1, y0, y1, z0, z1 = box or (0, nx, 0, ny, 0, nz)
    assert int(got.sum()) == (x1 - x0) * (y1 - y0) * (z1 - z0), what
    return got


# ---- 1. whole volumes ----

@pytest.mark.parametrize("dtype", ("f32", "f16"))
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_whole_volume_histograms_and_ranges(pkg, gpu, dims, dtype):
    upload_planes(pkg, dims, 4, dtype)
    pkg.bake_gradient(1)
    methods = (1, 2, 11, 13, G + 1)
    planes = {m: device_plane(pkg, m, dims) for m in methods}
    what = f"{dims} {dtype}"
    for m in methods:
        check_range(pkg, m, planes[m], what=what)
    win = {m: inner(planes[m]) for m in methods}
    # one plane: methods 1, 11 and 13; 1 bin, 9 x 1 bins, 256 bins
    check_hist(pkg, planes, 1, 1, what=what)
    check_hist(pkg, planes, 1, 9, what=what)
    check_hist(pkg, planes, 11, 9, win[11], what=what)
    check_hist(pkg, planes, 11, 256, what=what)
    check_hist(pkg, planes, 13, 1, win[13], what=what)
    check_hist(pkg, planes, 13, 9, what=what)
    # two planes: (1, 2), (13, 11), (1, gradient_of(1)) and u = v; 16 x 8, 64 x 64 (4
    # copies in LDS), 256 x 64 (the full 64 KiB, one copy), 1 x 1, 9 x 1 with a v plane
    check_hist(pkg, planes, 1, 16, None, 2, 8, None, what=what)
    check_hist(pkg, planes, 1, 256, win[1], 2, 64, win[2], what=what)
    check_hist(pkg, planes, 13, 16, win[13], 11, 8, win[11], what=what)
    check_hist(pkg, planes, 13, 1, None, 11, 1, None, what=what)
    check_hist(pkg, planes, 1, 256, None, pkg.gradient_of(1), 64, None, what=what)
    check_hist(pkg, planes, 1, 64, win[1], pkg.gradient_of(1), 64, win[G + 1], what=what)
    diag = check_hist(pkg, planes, 1, 16, win[1], 1, 16, win[1], what=what)
    assert int(np.trace(diag)) == planes[1].size  # u = v: the diagonal alone
    check_hist(pkg, planes, 2, 9, None, 1, 1, None, what=what)
    # default windows spread the plane over the table: both end bins are used
    if rh.window(planes[1])[1] != 1.0:
        h = pkg.plane_histogram(1, 16)
        assert h[0, 0] > 0 and h[0, -1] > 0, h


def test_codec_volume(pkg, gpu):
    """planes of the codec family: 4 with gradient_of(6), on the codec volume's grid"""
    pkg.init_codec(*codec_records())
    pkg.bake_stats()
    pkg.bake_gradient(6)
    g6 = pkg.gradient_of(6)
    planes = {m: device_plane(pkg, m, CODEC) for m in (4, g6)}
    for m in planes:
        check_range(pkg, m, planes[m], what="codec")
    check_hist(pkg, planes, 4, 16, None, g6, 8, None, what="codec")
    check_hist(pkg, planes, 4, 64, inner(planes[4]), g6, 64, inner(planes[g6]), what="codec")
    check_hist(pkg, planes, g6, 9, what="codec")
    box = (15, 22, 3, 4, 2, 9)
    check_hist(pkg, planes, 4, 16, None, g6, 8, None, box, what="codec box")
    check_range(pkg, 4, planes[4], box, what="codec box")


# ---- 2. boxes ----

BOX_DIMS = (37, 20, 11)
BOXES = {
    "one voxel": (36, 37, 19, 20, 10, 11),
    "the voxel x = 15": (15, 16, 6, 7, 3, 4),
    "from x = 15": (15, 37, 0, 20, 0, 11),
    "to x = 16": (0, 16, 0, 20, 0, 11),
    "to x = 15": (0, 15, 2, 20, 0, 11),
    "from x = 16": (16, 31, 0, 19, 1, 11),
    "the odd row of a pair": (0, 37, 7, 8, 0, 11),
    "the even row of a pair": (3, 33, 8, 9, 2, 9),
    "one slice": (0, 37, 0, 20, 4, 5),
    "inside": (7, 29, 5, 14, 3, 8),
    "the whole volume": (0, 37, 0, 20, 0, 11),
}


def test_boxes(pkg, gpu):
    upload_planes(pkg, BOX_DIMS, 4, "f32")
    planes = {m: device_plane(pkg, m, BOX_DIMS) for m in (1, 2)}
    w1, w2 = inner(planes[1]), inner(planes[2])
    whole = pkg.plane_histogram(1, 16, w1, 2, 8, w2)
    for name, box in BOXES.items():
        check_range(pkg, 1, planes[1], box, what=name)
        got = check_hist(pkg, planes, 1, 16, w1, 2, 8, w2, box, what=name)
        check_hist(pkg, planes, 2, 9, None, box=box, what=name)
        check_hist(pkg, planes, 1, 256, None, 2, 64, None, box, what=name)
        if name == "the whole volume":
            assert np.array_equal(got, whole)
    # two halves of a split at the apron add up to the whole
    a = pkg.plane_histogram(1, 16, w1, 2, 8, w2, box=(0, 15, 0, 20, 0, 11))
    b = pkg.plane_histogram(1, 16, w1, 2, 8, w2, box=(15, 37, 0, 20, 0, 11))
    assert np.array_equal(a + b, whole)


# ---- 3. values the bakes do not make, and slots that hold no voxel ----

def test_specials_and_poisoned_slots(pkg, gpu):
    """NaN, both infinities and both zeros written into the resident mean plane, and
    every float of the layout that is no voxel's home -- aprons, empty slots -- set to
    a value of a bin of its own: none of those may be counted"""
    dims = (37, 20, 11)
    upload_planes(pkg, dims, 4, "f32")
    ptr, n = plane_ptr(pkg, 1)
    home, floats = home_index(dims)
    flat = d2h(ptr, n, np.float32)
    rng = np.random.default_rng(2711)
    p = flat[home].copy()
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 2.0], np.float32)
    where = rng.choice(p.size, 70, replace=False)
    p.ravel()[where] = np.tile(specials, 10)
    poison = np.full(floats, 7.0, np.float32)  # bin 8 of 16 under (6.5, 1.0): no voxel's
    poison[home.ravel()] = p.ravel()
    h2d(ptr, poison)
    planes = {1: p, 2: device_plane(pkg, 2, dims)}
    got = check_range(pkg, 1, p, what="specials")
    assert got == (-np.inf, np.inf, 10)
    check_range(pkg, 1, p, (0, 16, 0, 20, 0, 11), what="specials")
    h = check_hist(pkg, planes, 1, 16, (6.5, 1.0), what="poison")
    assert h[0, 15] == 10 and h[0, 8] == 0 and h[0, 0] == p.size - 10  # +inf; no poison
    check_hist(pkg, planes, 1, 16, (0.0, 1.0), 2, 8, inner(planes[2]), what="specials")
    check_hist(pkg, planes, 1, 9, (0.25, -3.0), what="specials, a negative scale")
    check_hist(pkg, planes, 1, 9, (0.0, 0.0), what="specials, scale 0")
    for name in ("from x = 15", "to x = 16", "the odd row of a pair", "inside"):
        check_hist(pkg, planes, 1, 16, (0.0, 1.0), 2, 8, inner(planes[2]), BOXES[name], what=name)
    # every voxel NaN: the range is NaN
    allnan = np.full(floats, np.nan, np.float32)
    h2d(ptr, allnan)
    lo, hi, nn = pkg.plane_range(1)
    assert (bits(lo), bits(hi), nn) == (0x7FC00000, 0x7FC00000, p.size)
    assert int(pkg.plane_histogram(1, 4, (0.0, 1.0))[0, 0]) == p.size  # NaN: bin 0


# ---- 4. contention ----

def test_a_constant_plane_counts_exactly(pkg, gpu):
    """every voxel in one bin: the wave's pre-count and the copies in LDS add up"""
    dims = (70, 19, 67)
    upload_planes(pkg, dims, 4, "f32")
    voxels = 70 * 19 * 67
    for m in (1, 2):
        ptr, n = plane_ptr(pkg, m)
        h2d(ptr, np.full(n, 0.375 if m == 1 else 0.625, np.float32))
    planes = {1: np.full((67, 19, 70), 0.375, np.float32),
              2: np.full((67, 19, 70), 0.625, np.float32)}
    for nu in (256, 16384, 1):
        h = check_hist(pkg, planes, 1, nu, (0.0, 1.0), what="constant")
        assert int(h[0, int(0.375 * nu)]) == voxels
    for nu, nv in ((64, 64), (128, 128), (16, 8)):
        h = check_hist(pkg, planes, 1, nu, (0.0, 1.0), 2, nv, (0.0, 1.0), what="constant")
        assert int(h[int(0.625 * nv), int(0.375 * nu)]) == voxels
    assert pkg.plane_window(1) == (0.375, 1.0)  # max <= min
    assert int(pkg.plane_histogram(1, 9)[0, 0]) == voxels
    # and nearly constant: one voxel elsewhere breaks a wave's agreement once
    p = planes[1].copy()
    p[33, 7, 44] = 0.875
    home, floats = home_index(dims)
    flat = np.full(floats, 0.375, np.float32)
    flat[home.ravel()] = p.ravel()
    h2d(plane_ptr(pkg, 1)[0], flat)
    h = check_hist(pkg, {1: p, 2: planes[2]}, 1, 64, (0.0, 1.0), 2, 64, (0.0, 1.0), what="nearly")
    assert int(h[40, 56]) == 1 and int(h[40, 24]) == voxels - 1


# ---- 5. cross-checks with existing code ----

def test_cross_checks(pkg, gpu):
    import torch
    upload_planes(pkg, DIMS, 8, "f32")
    for m in (1, 11, 13):
        pkg.bake_gradient(m)
        lo, hi, nn = pkg.plane_range(pkg.gradient_of(m))
        assert bits(hi) == bits(pkg.gradient_info(m)[2]) and nn == 0 and lo >= 0
    # a frame under a set 2-D table, before and after: no state disturbed
    mx = pkg.gradient_info(1)[2]
    pkg.set_transfer_function_2d(RAND32, method_v=pkg.gradient_of(1), v_scale=float(f32(1) / f32(mx)))
    state = pkg.transfer_function_2d()
    cam = camera("C1")
    before = render(pkg, torch, cam, 1)
    info = pkg.layout_info()
    assert pkg.last_kernel() == kernel_of(1, G + 1)
    h = pkg.plane_histogram(1, 32, None, pkg.gradient_of(1), 32, (0.0, float(f32(1) / f32(mx))))
    assert pkg.last_kernel() == HIST1
    assert int(h.sum()) == DIMS[0] * DIMS[1] * DIMS[2]
    pkg.plane_range(2)
    assert pkg.last_kernel() == RANGE and pkg.plane_kernel_ms() > 0.0
    after = render(pkg, torch, cam, 1)
    assert pkg.last_kernel() == kernel_of(1, G + 1)
    assert_same(after, before, "a frame after a histogram")
    now = pkg.transfer_function_2d()
    assert np.array_equal(now[0], state[0]) and now[1:] == state[1:]
    assert pkg.layout_info() == info
    assert pkg.gradient_info(1)[2] == mx


# ---- 6. refusals ----

def _status(pkg, f):
    with pytest.raises(pkg.VRError) as e:
        f()
    return e.value.status, str(e.value)


def test_refusals(pkg, gpu):
    lib = pkg._lib
    pkg.init_distribution(volume(DIMS, 8, "f32"))
    # nothing baked: a state error with the bake's name, per plane
    for m, call in ((1, "vr_bake_stats"), (11, "vr_bake_quantile"), (13, "vr_bake_crossing"),
                    (G + 1, "vr_bake_gradient(1)")):
        for f in (lambda: pkg.plane_range(m), lambda: pkg.plane_histogram(m, 8, (0.0, 1.0)),
                  lambda: pkg.plane_histogram(m, 8)):
            st, msg = _status(pkg, f)
            assert st == lib.VR_ERR_STATE and call in msg, (m, msg)
    pkg.bake_stats()
    st, msg = _status(pkg, lambda: pkg.plane_histogram(1, 8, None, G + 2, 8))  # v not baked
    assert st == lib.VR_ERR_STATE and "vr_bake_gradient(2)" in msg
    whole = pkg.plane_histogram(1, 8, (0.0, 1.0), 2, 4, (0.0, 3.0))
    # a record plane with a codec plane
    for mu, mv in ((1, 4), (6, 2), (1, G + 5)):
        st, _ = _status(pkg, lambda: pkg.plane_histogram(mu, 8, (0.0, 1.0), mv, 4, (0.0, 1.0)))
        assert st == lib.VR_ERR_UNSUPPORTED, (mu, mv)
    # every argument error, with the planes resident
    nx, ny, nz = DIMS
    inf, nan = float("inf"), float("nan")
    bad = [lambda: pkg.plane_range(7), lambda: pkg.plane_range(0), lambda: pkg.plane_range(G + 7),
           lambda: pkg.plane_histogram(9, 8, (0.0, 1.0)),
           lambda: pkg.plane_histogram(1, 8, (0.0, 1.0), 7, 4, (0.0, 1.0)),
           lambda: pkg.plane_histogram(1, 0, (0.0, 1.0)),
           lambda: pkg.plane_histogram(1, 8, (0.0, 1.0), 2, 0, (0.0, 1.0)),
           lambda: pkg.plane_histogram(1, 16385, (0.0, 1.0)),
           lambda: pkg.plane_histogram(1, 129, (0.0, 1.0), 2, 128, (0.0, 1.0)),
           lambda: pkg.plane_histogram(1, 8, (0.0, 1.0), None, 2),
           lambda: pkg.plane_histogram(1, 8, (inf, 1.0)),
           lambda: pkg.plane_histogram(1, 8, (0.0, nan)),
           lambda: pkg.plane_histogram(1, 8, (0.0, 1.0), 2, 4, (0.0, -inf)),
           lambda: pkg.plane_histogram(1, 8, (0.0, 1.0), 2, 4, (nan, 1.0))]
    for box in ((0, 0, 0, ny, 0, nz), (5, 4, 0, ny, 0, nz), (0, nx, 3, 3, 0, nz),
                (0, nx, 0, ny, 9, 2), (-1, nx, 0, ny, 0, nz), (0, nx + 1, 0, ny, 0, nz),
                (0, nx, 0, ny + 1, 0, nz), (0, nx, 0, ny, 0, nz + 1), (nx, nx + 1, 0, 1, 0, 1)):
        bad.append(lambda box=box: pkg.plane_range(1, box))
        bad.append(lambda box=box: pkg.plane_histogram(1, 8, (0.0, 1.0), box=box))
    for k, f in enumerate(bad):
        st, msg = _status(pkg, f)
        assert st == lib.VR_ERR_ARG, (k, st, msg)
    buf = (ctypes.c_int * 6)(0, nx, 0, ny, 0, nz)
    assert lib.load().vr_plane_histogram(1, 0.0, 1.0, 8, 0, 0.0, 1.0, 1, ctypes.addressof(buf),
                                         None) == lib.VR_ERR_ARG
    lib.load().vr_clear_error()
    # a refused call changed nothing
    assert np.array_equal(pkg.plane_histogram(1, 8, (0.0, 1.0), 2, 4, (0.0, 3.0)), whole)
    # the planes gone: refused, not faulting
    pkg.freeCudaBuffers()
    for f in (lambda: pkg.plane_range(1), lambda: pkg.plane_histogram(1, 8, (0.0, 1.0)),
              lambda: pkg.plane_histogram(1, 8, (0.0, 1.0), 2, 4, (0.0, 1.0))):
        st, msg = _status(pkg, f)
        assert st == lib.VR_ERR_STATE and "vr_bake_stats" in msg
