"""The gradient-magnitude planes without a GPU: known answers
of the numpy restatement (tests/ref_gradient.py), its array form against its scalar
loop bit for bit, the host side of the C ABI (no device call), the reference frames
the GPU tests compare against with the conditions their scenes must meet, and a
census over mutants of the arithmetic: each must show in every test volume's plane
and in a frame."""
import ctypes
import functools

import numpy as np
import pytest

import ref_crossing
import ref_gradient
import ref_numpy
import ref_projection
import ref_shading
import ref_transfer
import ref_transfer2
from test_crossing import DIMS, H, W, camera
from test_shading import LIGHTS
from test_transfer import RAND256
from test_transfer2 import CODEC, RAND32, T255X4, blend_of, plane

f32 = np.float32
G = 32  # VR_QUERY_GRADIENT


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


# ---- known answers ----

def test_a_constant_plane_gives_plus_zero():
    for shape in ((1, 1, 1), (3, 4, 5), (1, 7, 2)):
        mag, mx = ref_gradient.gradient_plane(np.full(shape, 0.375, np.float32))
        assert not bits(mag).any() and bits(mx) == 0


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_a_ramp_gives_a_times_n_exactly(axis):
    """s = a * x with a a power of two: a * nx at every voxel, the faces included
    (the one-sided difference there is a * 1 * nx, the central one a * 2 * nx / 2);
    the same along y and z of a volume that is not a cube"""
    shape = (5, 6, 12)  # (nz, ny, nx)
    n = shape[axis]
    for a in (0.25, 2.0 ** -10, 8.0):
        idx = np.arange(n, dtype=np.float32).reshape([-1 if k == axis else 1 for k in range(3)])
        s = np.broadcast_to(f32(a) * idx, shape).astype(np.float32)
        mag, mx = ref_gradient.gradient_plane(s)
        assert np.all(mag == f32(a) * f32(n)) and mx == f32(a) * f32(n)
        # and no mutant gives that
        for mutant in ref_gradient.MUTANTS:
            assert not np.array_equal(ref_gradient.gradient_plane(s, mutant)[0], mag), mutant


def test_an_axis_of_one_voxel_contributes_nothing():
    rng = np.random.default_rng(2701)
    s = rng.random((1, 6, 9)).astype(np.float32)
    flat, _ = ref_gradient.gradient_plane(s)
    thick, _ = ref_gradient.gradient_plane(np.repeat(s, 3, axis=0))  # constant along z
    assert np.array_equal(bits(flat[0]), bits(thick[1]))
    line, _ = ref_gradient.gradient_plane(s[:, :1, :])
    want = np.abs(np.gradient(s[0, 0].astype(np.float64)) * 9)
    assert np.allclose(line[0, 0, 1:-1], want[1:-1], rtol=1e-6)
    assert not bits(ref_gradient.gradient_plane(s[:, :1, :1])[0]).any()


@pytest.mark.parametrize("shape", ((1, 1, 1), (1, 2, 16), (3, 1, 15), (5, 9, 31), (4, 5, 7)))
def test_the_array_form_is_the_scalar_loop(shape):
    rng = np.random.default_rng(2702)
    s = (rng.random(shape) * 2 - 0.5).astype(np.float32)
    a, amax = ref_gradient.gradient_plane(s)
    b, bmax = ref_gradient.gradient_plane_scalar(s)
    assert np.array_equal(bits(a), bits(b)) and bits(amax) == bits(bmax)
    assert amax == a.max()


# ---- ABI and setters, no device call ----

SOURCES = (1, 2, 3, 4, 5, 6, 10, 11, 12, 13)


def _state(pkg):
    t = pkg.transfer_function_2d()
    return None if t is None else (t[0].tobytes(), t[0].shape) + t[1:]


def _set(L, tab, mv):
    tab = np.ascontiguousarray(tab, dtype=np.float32)
    return L.vr_set_transfer_function_2d(tab.ctypes.data, tab.shape[1], tab.shape[0], mv, 0.0, 1.0)


def test_gradient_state_without_gpu(pkg):
    L, lib = pkg._lib.load(), pkg._lib
    assert lib.VR_QUERY_GRADIENT == pkg.GRADIENT == G
    assert [pkg.gradient_of(m) for m in SOURCES] == [G + m for m in SOURCES]
    for m in (0, 7, 9, 14, 32):
        with pytest.raises(ValueError):
            pkg.gradient_of(m)
    pkg.freeCudaBuffers()
    pkg.set_transfer_function_2d(None)
    L.vr_clear_error()
    # the ten values are method_v's, everything else is still refused
    for m in SOURCES:
        pkg.set_transfer_function_2d(RAND32, method_v=pkg.gradient_of(m), v_scale=0.5)
        assert pkg.transfer_function_2d()[1:] == (G + m, 0.0, 0.5)
    keep = _state(pkg)
    for mv in (0, 7, 8, 9, 14, 31, 32, 39, 46, -1):
        assert _set(L, RAND32, mv) == lib.VR_ERR_ARG, mv
        assert _state(pkg) == keep, mv
    pkg.set_transfer_function_2d(None)
    # the bake: an argument error, then a state error that names the source's bake
    for m in (7, 0, 14, 32, -1):
        assert L.vr_bake_gradient(m) == lib.VR_ERR_ARG
        assert L.vr_release_gradient(m) == lib.VR_ERR_ARG
        assert L.vr_gradient_info(m, None, None, None) == lib.VR_ERR_ARG
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_gradient(7)
    assert e.value.status == lib.VR_ERR_ARG
    for m, call in ((1, "vr_bake_stats"), (5, "vr_bake_stats"), (10, "vr_bake_weighted"),
                    (11, "vr_bake_quantile"), (12, "vr_bake_distance"), (13, "vr_bake_crossing")):
        with pytest.raises(pkg.VRError) as e:
            pkg.bake_gradient(m)
        assert e.value.status == lib.VR_ERR_STATE and call in str(e.value), str(e.value)
    for m in SOURCES:
        assert pkg.gradient_info(m) == (None, 0, 0.0)
        pkg.release_gradient(m)  # nothing there: nothing to do
    L.vr_clear_error()


def test_a_frame_of_an_unbaked_gradient_plane_is_refused(pkg):
    """before the library looks for a volume: a gradient method has no per-step march"""
    L, lib = pkg._lib.load(), pkg._lib
    pkg.freeCudaBuffers()
    for m in (1, 5, 13):
        d = pkg.make_desc(0x1000, W, H, camera("C0"), query_method=G + m, volume_size=(4, 4, 4))
        assert L.vr_render(ctypes.byref(d)) == lib.VR_ERR_UNSUPPORTED
        assert "vr_bake_gradient" in L.vr_last_error().decode()
        for call in (L.vr_count_footprint, L.vr_footprint_bytes):
            assert call(ctypes.byref(d)) == lib.VR_ERR_UNSUPPORTED
            assert "vr_bake_gradient" in L.vr_last_error().decode()
        assert L.vr_render_gmm_baked(ctypes.byref(d)) == lib.VR_ERR_UNSUPPORTED
    d = pkg.make_desc(0x1000, W, H, camera("C0"), query_method=G + 7, volume_size=(4, 4, 4))
    assert L.vr_render(ctypes.byref(d)) in (lib.VR_ERR_ARG, lib.VR_ERR_STATE)
    L.vr_clear_error()


def test_exports(pkg):
    for name in ("GRADIENT", "gradient_of", "bake_gradient", "release_gradient", "gradient_info"):
        assert name in pkg.api.__all__ and hasattr(pkg, name), name
    for name in ("vr_bake_gradient", "vr_release_gradient", "vr_gradient_info"):
        assert name in pkg._lib.EXPORTS and hasattr(pkg._lib.load(), name), name


# ---- the volumes and frames of the GPU tests (tests/test_gpu_gradient.py) ----

# the shapes whose planes the GPU test checks voxel by voxel, as (nx, ny, nz).  The
# kernel's tile is 4 bricks (60 voxels of x and the last brick's apron) by 8 y pairs
# (16 rows) and a z chunk is 64 slices: the last shape has two tiles in x, two in y
# and two chunks
PLANE_SHAPES = ((1, 1, 1), (16, 2, 1), (15, 1, 3), (31, 9, 5), (37, 20, 11), (70, 19, 67))


@functools.lru_cache(maxsize=None)
def gplane(dims, nb, dtype, src, mutant=None):
    """(|grad| of test_transfer2.plane(dims, nb, dtype, src), its maximum); read-only"""
    mag, mx = ref_gradient.gradient_plane(plane(dims, nb, dtype, src), mutant)
    mag.setflags(write=False)
    return mag, mx


def any_plane(dims, nb, dtype, method, mutant=None):
    if method > G:
        return gplane(dims, nb, dtype, method - G, mutant)[0]
    return plane(dims, nb, dtype, method)


def inv_max(dims, nb, dtype, src):
    """1 / max as the GPU tests compute it from gradient_info: float32"""
    return float(f32(1) / gplane(dims, nb, dtype, src)[1])


# name -> what the frame is.  kind tf1: a 1-D table; tf2: a 2-D table over (u, v), the
# window of a gradient axis 1 / max of its plane; proj: a projection; lit: the light;
# plain: nothing set (the built-in table).  All on DIMS x 8 (24 x 20 x 16: no cube)
# but the codec pair, on CODEC (22 x 18 x 14)
FRAMES = {
    "tf1": dict(kind="tf1", dims=DIMS, u=G + 1, table="rand256"),
    "kniss": dict(kind="tf2", dims=DIMS, u=1, v=G + 1, table="rand32"),
    "other": dict(kind="tf2", dims=DIMS, u=13, v=G + 10, table="t255x4"),
    "grad-u": dict(kind="tf2", dims=DIMS, u=G + 13, v=2, voff=0.08, vscale=3.0, table="rand32"),
    "codec": dict(kind="tf2", dims=CODEC, u=4, v=G + 6, table="rand32"),
    "proj": dict(kind="proj", dims=DIMS, u=G + 11, mode="max"),
    "lit": dict(kind="lit", dims=DIMS, u=G + 10, table="rand256", light=LIGHTS[1]),
    "plain": dict(kind="plain", dims=DIMS, u=G + 2),
}
TABLES1 = {"rand256": RAND256}
TABLES2 = {"rand32": RAND32, "t255x4": T255X4}
CAMS = ("C0", "C1")


def windows(f, dtype):
    """(toff, tscale, voff, vscale) of frame f: 1 / max on a gradient axis"""
    u, v = f["u"], f.get("v")
    tscale = inv_max(f["dims"], 8, dtype, u - G) if u > G else 1.0
    if v is None:
        return 0.0, tscale, 0.0, 1.0
    vscale = inv_max(f["dims"], 8, dtype, v - G) if v > G else f["vscale"]
    return 0.0, tscale, f.get("voff", 0.0), vscale


@functools.lru_cache(maxsize=None)
def reference(name, dtype, cam, mutant=None, row0=False):
    """the numpy frame `name` of the GPU tests, computed once and shared: (RGBA8, float
    RGBA, samples), read-only.  mutant: with the gradient plane of that mutant (the
    windows stay the right plane's); row0: a 2-D table with every row its row 0."""
    f = FRAMES[name]
    dims, m = f["dims"], camera(cam)
    toff, tscale, voff, vscale = windows(f, dtype)
    pu = any_plane(dims, 8, dtype, f["u"], mutant)
    kw = dict(toff=toff, tscale=tscale)
    if f["kind"] == "tf1":
        ref = ref_transfer.render_plane(pu, W, H, m, TABLES1[f["table"]],
                                        blend=ref_crossing.trilinear, **kw)
    elif f["kind"] == "plain":
        ref = ref_transfer.render_plane(pu, W, H, m, ref_numpy.TF, blend=ref_crossing.trilinear,
                                        **kw)
    elif f["kind"] == "proj":
        ref = ref_projection.render_plane(pu, W, H, m, f["mode"], blend=ref_crossing.trilinear, **kw)
    elif f["kind"] == "lit":
        ref = ref_shading.render_plane(pu, W, H, m, TABLES1[f["table"]], f["light"],
                                       blend=ref_crossing.trilinear, **kw)
    else:
        tab = TABLES2[f["table"]]
        if row0:
            tab = np.repeat(tab[:1], tab.shape[0], axis=0)
        ref = ref_transfer2.render_planes(pu, any_plane(dims, 8, dtype, f["v"], mutant), W, H, m,
                                          tab, blend_u=blend_of(f["u"]), blend_v=blend_of(f["v"]),
                                          voff=voff, vscale=vscale, **kw)
    for a in ref:
        a.setflags(write=False)
    return tuple(ref)


@pytest.mark.parametrize("cam", CAMS)
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_reference_frame_is_worth_comparing(name, cam):
    """more than 1000 pixels are hit, and in a 2-D frame at least a quarter of them
    differ from the frame whose table has its v rows all equal to row 0"""
    rgba8, _, steps = reference(name, "f32", cam)
    hit = steps >= 0
    assert hit.sum() > 1000, int(hit.sum())
    assert np.unique(rgba8[hit]).size > 50
    if FRAMES[name]["kind"] == "tf2":
        flat = reference(name, "f32", cam, row0=True)
        differ = (rgba8 != flat[0]) & hit
        assert 4 * differ.sum() >= hit.sum(), (int(differ.sum()), int(hit.sum()))


def test_the_built_in_table_is_the_reference_table(pkg):
    """the frame with nothing set is the 1-D table frame of REFERENCE_TF"""
    assert np.array_equal(np.asarray(pkg.REFERENCE_TF, np.float32), ref_numpy.TF.astype(np.float32))


# ---- census over mutants ----

def _volume_planes():
    """a source plane for every shape of the GPU plane test: seeded, smooth along no axis"""
    for nx, ny, nz in PLANE_SHAPES:
        rng = np.random.default_rng(2703 + nx)
        yield (nx, ny, nz), rng.random((nz, ny, nx)).astype(np.float32)
    yield DIMS, plane(DIMS, 8, "f32", 1)
    yield CODEC, plane(CODEC, 8, "f32", 6)


@pytest.mark.parametrize("mutant", ref_gradient.MUTANTS)
def test_every_mutant_shows(mutant):
    """in the plane of every test volume with more than one voxel, and in a pixel of a
    GPU test frame"""
    for dims, s in _volume_planes():
        right, _ = ref_gradient.gradient_plane(s)
        wrong, _ = ref_gradient.gradient_plane(s, mutant)
        if dims == (1, 1, 1):  # one voxel: every version gives +0
            assert not bits(right).any() and not bits(wrong).any()
            continue
        assert not np.array_equal(bits(right), bits(wrong)), (mutant, dims)
    shown = 0
    for name in ("tf1", "kniss"):
        right = reference(name, "f32", "C1")
        wrong = reference(name, "f32", "C1", mutant=mutant)
        shown += int((right[0] != wrong[0]).sum())
    assert shown > 0, mutant
