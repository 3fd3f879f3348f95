"""Headlight gradient shading without a GPU: the numpy march
(tests/ref_shading.py) against its scalar restatement, its tie to the existing
reference (the identity light is ref_transfer's frame; no light changes a ray's
length), known answers of the gradient, the host state of the C ABI (vr_set_light
makes no device call), and the reference frames the GPU tests compare against with a
census that keeps them worth comparing."""
import ctypes
import functools

import numpy as np
import pytest

import ref_numpy
import ref_shading
import ref_transfer
from ref_numpy import _lin
from test_crossing import BAKE, DIMS, H, W, camera, cdf
from test_transfer import BLENDS, RAMP2, RAND256, TABLES

f32 = np.float32
VIEWS = ("C0", "C1", "S")
# (ka, kd, ks, k): matte, a highlight of exponent 16, no ambient and exponent 128
LIGHTS = ((0.3, 0.7, 0.0, 0), (0.2, 0.5, 0.6, 4), (0.0, 1.0, 1.0, 7))
IDENTITY = ref_shading.IDENTITY


def table_of(name):
    return None if name is None else TABLES[name]


# ---- the reference frames of the GPU tests ----

@functools.lru_cache(maxsize=None)
def reference(dims, nb, dtype, cam, w, h, table, blend, light):
    """the numpy frame lit by `light` under TABLES[table] (None: the built-in table)
    with BLENDS[blend] over the plane of F of test_crossing.cdf, computed once per case
    and shared by the CPU and the GPU tests: (RGBA8, float RGBA, samples, info), arrays
    read-only"""
    info = {}
    ref = ref_shading.render_plane(cdf(dims, nb, dtype), w, h, camera(cam), table_of(table),
                                   light, blend=BLENDS[blend], info=info)
    for a in ref:
        a.setflags(write=False)
    return ref + (info,)


@functools.lru_cache(maxsize=None)
def unlit(dims, nb, dtype, cam, w, h, table, blend):
    """the same frame without the light, by ref_transfer (None: under ref_numpy.TF)"""
    ref = ref_transfer.render_plane(cdf(dims, nb, dtype), w, h, camera(cam),
                                    ref_numpy.TF if table is None else TABLES[table],
                                    blend=BLENDS[blend])
    for a in ref:
        a.setflags(write=False)
    return ref


# ---- the scalar restatement ----

@pytest.mark.parametrize("blend", sorted(BLENDS))
def test_scalar_loop_is_the_array_march(blend):
    """20 seeded pixels, one ray at a time in Python scalars"""
    F, m = cdf(DIMS, 8, "f32"), camera("C1")
    kw = dict(blend=BLENDS[blend], density=0.07, brightness=1.25, toff=0.05, tscale=1.5)
    light = (0.2, 0.5, 0.6, 4)
    _, rgba, n = ref_shading.render_plane(F, W, H, m, RAND256, light, **kw)
    rng = np.random.default_rng(2501)
    ys, xs = np.nonzero(n >= 0)
    pick = rng.choice(ys.size, 17, replace=False)
    pixels = [(int(xs[i]), int(ys[i])) for i in pick] + [(0, 0), (W - 1, H - 1), (W // 2, 0)]
    hits = 0
    for x, y in pixels:
        got, gn = ref_shading.render_ray(F, W, H, m, x, y, RAND256, light, **kw)
        assert gn == n[y, x], (x, y)
        if gn < 0:
            continue
        hits += 1
        assert got.tobytes() == rgba[y, x].tobytes(), (x, y)
    assert hits >= 17


# ---- the tie to the existing reference ----

@pytest.mark.parametrize("blend", sorted(BLENDS))
def test_identity_light_is_the_unlit_frame(blend):
    """(ka, kd, ks) = (1, 0, 0): shade is exactly 1, spec exactly +0"""
    for dims, nb, cam, table in ((DIMS, 8, "C1", "rand256"), (DIMS, 8, "C0", None),
                                 (BAKE, 4, "S", "ramp2")):
        for k in (0, 7):
            got = ref_shading.render_plane(cdf(dims, nb, "f32"), W, H, camera(cam), table_of(table),
                                           (1.0, 0.0, 0.0, k), blend=BLENDS[blend])
            want = unlit(dims, nb, "f32", cam, W, H, table, blend)
            assert (want[2] >= 0).sum() > 500
            for g, r in zip(got, want):
                assert g.dtype == r.dtype and np.array_equal(g, r), (dims, cam, table, k)


@pytest.mark.parametrize("blend", sorted(BLENDS))
def test_samples_per_pixel_are_the_unlit_frame_s(blend):
    """opacity is not lit: every ray ends where it ends without the light"""
    for dims, nb in ((DIMS, 8), (BAKE, 4)):
        for cam in VIEWS:
            want = unlit(dims, nb, "f32", cam, W, H, "rand256", blend)
            for light in LIGHTS:
                got = reference(dims, nb, "f32", cam, W, H, "rand256", blend, light)
                assert np.array_equal(got[2], want[2]), (dims, cam, light)
                assert np.array_equal(got[1][..., 3], want[1][..., 3]), (dims, cam, light)


# ---- known answers ----

@pytest.mark.parametrize("blend", sorted(BLENDS))
def test_constant_plane(blend):
    """no cell has a gradient, so c = 1 everywhere: shade = ka + kd and spec = ks.  With
    ka + kd = 1 and ks = 0 that is the unlit frame; otherwise the frame of the light
    (ka + kd, 0, 0), whose shade is the same float"""
    F = np.full(DIMS[::-1], f32(0.3125), np.float32)
    m = camera("C1")
    info = {}
    got = ref_shading.render_plane(F, W, H, m, RAND256, (0.25, 0.75, 0.0, 3), blend=BLENDS[blend],
                                   info=info)
    want = ref_transfer.render_plane(F, W, H, m, RAND256, blend=BLENDS[blend])
    assert info["flat"] == info["samples"] > 10000 and np.all(info["c"] == 1)
    for g, r in zip(got, want):
        assert np.array_equal(g, r)
    a = ref_shading.render_plane(F, W, H, m, RAND256, (0.3, 0.5, 0.0, 2), blend=BLENDS[blend])
    b = ref_shading.render_plane(F, W, H, m, RAND256, (f32(0.3) + f32(0.5), 0.0, 0.0, 0),
                                 blend=BLENDS[blend])
    for g, r in zip(a, b):
        assert np.array_equal(g, r)
    assert (a[0] != want[0]).sum() > 500
    # the highlight of a flat cell is ks itself, whatever the exponent
    p = ref_shading.render_plane(F, W, H, m, RAND256, (0.3, 0.5, 0.25, 0), blend=BLENDS[blend])
    q = ref_shading.render_plane(F, W, H, m, RAND256, (0.3, 0.5, 0.25, 7), blend=BLENDS[blend])
    assert np.array_equal(p[0], q[0]) and (p[0] != a[0]).sum() > 500


def test_plane_linear_in_x():
    """F = x / 64: Gx = nx / 64 in every cell whose x pair is two voxels, 0 in the
    clamped rim, and Gy = Gz = 0 everywhere -- exactly"""
    nx, ny, nz = DIMS
    F = np.broadcast_to(np.arange(nx, dtype=np.float32) * f32(1 / 64), (nz, ny, nx))
    rng = np.random.default_rng(2502)
    u = rng.random((3, 4000)).astype(np.float32)
    u[:, :200] = rng.choice(f32([0, 1, 0.001, 0.999]), (3, 200))  # the rim
    ax = [_lin(u[k], DIMS[k]) for k in range(3)]
    vals = np.stack([F[ax[2][1 if j & 4 else 0], ax[1][1 if j & 2 else 0], ax[0][1 if j & 1 else 0]]
                     for j in range(8)])
    Gx, Gy, Gz = ref_shading.gradient(vals, ax, DIMS)
    inner = ax[0][0] != ax[0][1]
    assert 3000 < inner.sum() < 4000
    assert np.all(Gx[inner] == f32(nx) / f32(64)) and np.all(Gx[~inner] == 0)
    assert not Gy.any() and not Gz.any()
    # a ray along x sees c = 1, a ray across it c = 0
    one = np.ones_like(Gx)
    c = ref_shading.cosine((Gx, Gy, Gz), (one, 0 * one, 0 * one))
    assert np.all(c == 1)
    c = ref_shading.cosine((Gx, Gy, Gz), (0 * one, one, 0 * one))
    assert np.all(c[inner] == 0) and np.all(c[~inner] == 1)


def test_shade_known_answers():
    c = f32([0.0, 0.5, 1.0])
    sh, sp = ref_shading.shade(c, (0.25, 0.5, 2.0, 3))
    assert np.array_equal(sh, f32([0.25, 0.5, 0.75]))
    assert np.array_equal(sp, f32([0.0, 2.0 ** -7, 2.0]))  # c ** 8
    sh, sp = ref_shading.shade(c, IDENTITY)
    assert np.all(sh == 1) and not sp.any() and not np.signbit(sp).any()
    # a NaN cosine cannot arise: cosine() returns 1 for it
    nan = f32([np.nan])
    assert ref_shading.cosine((nan, nan, nan), (nan, nan, nan))[0] == 1
    big = f32([3e38])
    assert ref_shading.cosine((big, big, big), (big, big, big))[0] == 1  # inf / inf


# ---- the census of the reference frames ----

@pytest.mark.parametrize("cam", VIEWS)
@pytest.mark.parametrize("dims,nb", ((DIMS, 8), (BAKE, 4)), ids=("DIMS", "BAKE"))
def test_reference_frames_are_worth_comparing(dims, nb, cam):
    """by the reference alone, for both blends, under rand256 and under no table, the
    three lights of the GPU test: the lit and the unlit RGBA8 differ in at least a third
    of the hit pixels; c < 0.5 in at least 5 % of the samples and c > 0.9 in at least
    5 %; cells without a gradient occur, in fewer than half of the samples; and the
    highlight of (ks = 0.6, k = 4) changes at least 20 pixels"""
    for blend in sorted(BLENDS):
        for table in ("rand256", None):
            base = unlit(dims, nb, "f32", cam, W, H, table, blend)
            hit = base[2] >= 0
            for light in LIGHTS:
                rgba8, _, n, info = reference(dims, nb, "f32", cam, W, H, table, blend, light)
                c = info["c"]
                differ = int((rgba8 != base[0])[hit].sum())
                print(dims, cam, blend, table, light, int(hit.sum()), differ,
                      round(float((c < 0.5).mean()), 3), round(float((c > 0.9).mean()), 3),
                      info["flat"], info["samples"])
                assert np.array_equal(n, base[2])
                assert 3 * differ >= hit.sum() > 1000
                assert c.size == info["samples"]
                assert (c < 0.5).mean() >= 0.05 and (c > 0.9).mean() >= 0.05
                assert 0 < info["flat"] < info["samples"] / 2
            ka, kd, ks, k = LIGHTS[1]
            assert ks > 0 and k == 4
            matte = ref_shading.render_plane(cdf(dims, nb, "f32"), W, H, camera(cam),
                                             table_of(table), (ka, kd, 0.0, k), blend=BLENDS[blend])
            shiny = reference(dims, nb, "f32", cam, W, H, table, blend, LIGHTS[1])
            assert (matte[0] != shiny[0]).sum() >= 20


# ---- host state of the C ABI ----

def test_light_state_without_gpu(pkg):
    L, lib = pkg._lib.load(), pkg._lib
    pkg.freeCudaBuffers()
    pkg.set_light(None)
    L.vr_clear_error()
    assert pkg.light() is None and L.vr_light_state(None) == 0
    try:
        # the defaults, read back, replace
        pkg.set_light()
        assert pkg.light() == {"ambient": f32(0.3), "diffuse": f32(0.7), "specular": 0.0,
                               "shininess": 1}
        assert L.vr_light_state(None) == 1
        for s in (1, 2, 4, 8, 16, 32, 64, 128):
            pkg.set_light(0.0, 1.5, 2.0, s)
            got = lib.Light()
            assert L.vr_light_state(ctypes.byref(got)) == 1
            assert (got.ambient, got.diffuse, got.specular) == (0.0, 1.5, 2.0)
            assert got.shininess_log2 == s.bit_length() - 1 and pkg.light()["shininess"] == s
        pkg.set_light(ambient=1.0, diffuse=0.0)
        assert pkg.light() == {"ambient": 1.0, "diffuse": 0.0, "specular": 0.0, "shininess": 1}
        # errors leave the state as it was
        pkg.set_light(0.25, 0.5, 0.125, 16)
        keep = pkg.light()
        for bad in (0, 3, 5, 129, 256, -2, 2.0, "4", True, None):
            with pytest.raises(ValueError):
                pkg.set_light(0.1, 0.1, 0.1, bad)
            assert pkg.light() == keep
        for bad in (np.nan, np.inf, -np.inf, -1e-30, -1.0):
            for where in range(3):
                v = [0.1, 0.2, 0.3]
                v[where] = bad
                with pytest.raises(pkg.VRError) as e:
                    pkg.set_light(*v, 4)
                assert e.value.status == lib.VR_ERR_ARG
                assert ("ambient", "diffuse", "specular")[where] in str(e.value)
                assert pkg.light() == keep
        for k in (-1, 8, 1 << 20):
            raw = lib.Light(0.1, 0.2, 0.3, k)
            assert L.vr_set_light(ctypes.byref(raw)) == lib.VR_ERR_ARG
            assert "shininess_log2" in L.vr_last_error().decode()
            assert pkg.light() == keep
        L.vr_clear_error()
        # the light is the caller's: it outlives freeCudaBuffers, the releases and the
        # other setters; nothing so far has made a device call
        pkg.freeCudaBuffers()
        pkg.release_stats()
        pkg.release_crossing()
        pkg.release_weighted()
        pkg.release_gmm_stats()
        pkg.set_bin_weights([1.0, 2.0])
        pkg.set_bin_weights(None)
        pkg.set_transfer_function(RAMP2)
        pkg.set_transfer_function(None)
        pkg.set_transfer_function_2d(np.zeros((2, 2, 4), np.float32), 1)
        pkg.set_transfer_function_2d(None)
        pkg.set_projection("max")
        pkg.set_projection(None)
        assert pkg.light() == keep
        L.vr_clear_error()
        pkg.set_light(0.5, 0.5)
        assert L.vr_last_status() == lib.VR_OK and L.vr_last_error() == b""
        # only a NULL call clears it
        assert L.vr_set_light(None) == lib.VR_OK
        assert pkg.light() is None
    finally:
        pkg.set_light(None)
        pkg.set_projection(None)
        pkg.set_transfer_function(None)
        pkg.set_transfer_function_2d(None)
        L.vr_clear_error()


def test_refusals_come_before_any_device_work(pkg):
    """with the light on, what has no lit plane march is refused outright -- the counts
    before they look at their descriptor"""
    L, lib = pkg._lib.load(), pkg._lib
    pkg.freeCudaBuffers()
    d = pkg.make_desc(0x1000, W, H, camera("C0"), query_method=1, volume_size=(4, 4, 4))
    try:
        pkg.set_light(0.2, 0.5, 0.6, 16)
        for call in (L.vr_count_footprint, L.vr_footprint_bytes, L.vr_gmm_count_footprint):
            assert call(ctypes.byref(d)) == lib.VR_ERR_UNSUPPORTED
            msg = L.vr_last_error().decode()
            assert "light" in msg and "bake" in msg and "vr_set_light(NULL)" in msg, msg
        assert L.vr_gmm_count_footprint_slab(ctypes.byref(d), None) == lib.VR_ERR_UNSUPPORTED
        assert L.vr_render_gmm(ctypes.byref(d), None) == lib.VR_ERR_UNSUPPORTED
        assert "vr_set_light(NULL)" in L.vr_last_error().decode()
        for method in (1, 2, 10, 11, 13):  # no baked GMM plane
            d.query_method = method
            assert L.vr_render_gmm_baked(ctypes.byref(d)) == lib.VR_ERR_UNSUPPORTED
            assert "vr_set_light(NULL)" in L.vr_last_error().decode()
        d.query_method = 1
        # a projection at the same time: the light's refusal, and it says why
        pkg.set_projection("max")
        assert L.vr_count_footprint(ctypes.byref(d)) == lib.VR_ERR_UNSUPPORTED
        msg = L.vr_last_error().decode()
        assert "once per ray" in msg and "vr_set_light(NULL)" in msg, msg
        assert "vr_set_projection(0)" in msg, msg
        pkg.set_projection(None)
        # a 2-D table at the same time
        pkg.set_transfer_function_2d(np.zeros((2, 2, 4), np.float32), 1)
        assert L.vr_count_footprint(ctypes.byref(d)) == lib.VR_ERR_UNSUPPORTED
        msg = L.vr_last_error().decode()
        assert "2-D transfer function" in msg and "vr_set_light(NULL)" in msg, msg
    finally:
        pkg.set_light(None)
        pkg.set_projection(None)
        pkg.set_transfer_function_2d(None)
        L.vr_clear_error()
    # cleared: the usual state error of a library without a volume
    assert L.vr_count_footprint(ctypes.byref(d)) == lib.VR_ERR_STATE
    L.vr_clear_error()


def test_exports(pkg):
    for name in ("set_light", "light"):
        assert name in pkg.api.__all__ and hasattr(pkg, name), name
    for name in ("vr_set_light", "vr_light_state"):
        assert name in pkg._lib.EXPORTS and hasattr(pkg._lib.load(), name), name
    assert ctypes.sizeof(pkg._lib.Light) == 16
