"""GPU checks of headlight gradient shading (vr_shade.hip).

The march, the gradient, the cosine with its one square root and one division, and
the lit classification are float arithmetic in a fixed order which numpy float32
restates bit for bit (tests/ref_shading.py), so every comparison is exact: packed
RGBA8, float RGBA and samples per pixel are np.array_equal, no tolerance and no pixel
left out.  The reference frames are test_shading.py's, which that file checks on the
CPU.  The shapes are small on purpose: BAKE's 5 x 3 rows clamp footprints (cells with
no gradient along an axis), DIMS has rays of one sample and of 296, and 70 x 50 is no
multiple of the 64 x 4 tile.
"""
import numpy as np
import pytest

import ref_shading
from test_crossing import BAKE, DIMS, H, THETA, W, camera, cdf, volume
from test_gpu_crossing import GH, GW, PAD, SENTINEL, assert_same, gmm_records, render
from test_gpu_transfer import TF_BLEND, TF_CROSS, bake_gmm_planes, gmm_frame, upload_F_planes
from test_shading import IDENTITY, LIGHTS, reference, unlit
from test_transfer import BLENDS, RAMP2, RAND256, TABLES

pytestmark = pytest.mark.gpu

# the two planes of F the numpy frames are marched over: method 10's (blended) and
# method 13's (combined)
PLANES = ((10, "trilinear", False), (13, "combine", True))


def kernel(cross):
    return f"k_march_lit<B=1,M={13 if cross else 0}>"


def set_light(pkg, light):
    ka, kd, ks, k = light
    pkg.set_light(ka, kd, ks, 1 << k)


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
        pkg.clear_gmm_range()
        pkg.set_stream(None)
        pkg.clear_tuning()
    clear()
    pkg.freeCudaBuffers()
    yield
    clear()
    pkg.freeCudaBuffers()


def set_table(pkg, name):
    pkg.set_transfer_function(None if name is None else TABLES[name])


# ---- 1. against numpy ----

NUMPY_CASES = (
    [(DIMS, 8, dt, cam, w, h) for dt in ("f32", "f16")
     for cam, w, h in (("C0", W, H), ("C1", W, H), ("S", W, H), ("C1", 70, 50))]
    + [(BAKE, 4, "f32", cam, W, H) for cam in ("C0", "C1", "S")]
)


@pytest.mark.parametrize("table", ("ramp2", "rand256", "one", "n255", None))
@pytest.mark.parametrize("case", NUMPY_CASES, ids=lambda c: "-".join(
    "x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c))
def test_against_numpy(pkg, gpu, case, table):
    """the three lights on the method-10 and the method-13 plane"""
    import torch
    dims, nb, dtype, cam, w, h = case
    upload_F_planes(pkg, dims, nb, dtype)
    set_table(pkg, table)
    for light in LIGHTS:
        set_light(pkg, light)
        for method, blend, cross in PLANES:
            got = render(pkg, torch, w, h, camera(cam), method=method)
            assert pkg.last_kernel() == kernel(cross)
            assert_same(got, reference(dims, nb, dtype, cam, w, h, table, blend, light)[:3],
                        f"{light} {table} method {method} {case}")
    assert pkg.layout_info()["resident_bytes"] == 0  # no layout copy is used or made


# ---- 2. both addressing modes ----

def test_wide_addressing_changes_no_pixel(pkg, gpu, tune):
    import torch
    for dims, nb, dtype in ((DIMS, 8, "f32"), (BAKE, 4, "f32")):
        upload_F_planes(pkg, dims, nb, dtype)
        pkg.set_transfer_function(RAND256)
        set_light(pkg, LIGHTS[1])
        for method, blend, cross in PLANES:
            tune.clear("VR_TF_WIDE")
            narrow = render(pkg, torch, W, H, camera("C1"), method=method)
            tune.set("VR_TF_WIDE", "1")
            wide = render(pkg, torch, W, H, camera("C1"), method=method)
            assert pkg.last_kernel() == kernel(cross)
            assert_same(wide, narrow, f"VR_TF_WIDE {dims} method {method}")
            assert_same(wide, reference(dims, nb, dtype, "C1", W, H, "rand256", blend,
                                        LIGHTS[1])[:3], "wide")
        tune.clear("VR_TF_WIDE")


# ---- 3. the identity light is the k_march_plane_tf frame ----

def identity(pkg, frame, cross, what):
    """under a caller's table, and with none (the built-in nine through rtf_upload)
    against the table march of the reference's nine entries"""
    for table in (RAND256, pkg.REFERENCE_TF):
        pkg.set_light(None)
        pkg.set_transfer_function(table)
        copies = pkg.layout_info()["resident_bytes"]
        want = frame()
        assert pkg.last_kernel() == (TF_CROSS if cross else TF_BLEND), (what, pkg.last_kernel())
        assert (want[2] >= 0).sum() > 100, what
        lit_tables = (table,) if table is RAND256 else (table, None)
        for lit_table in lit_tables:
            pkg.set_transfer_function(lit_table)
            for k in (1, 128):
                pkg.set_light(1.0, 0.0, 0.0, k)
                got = frame()
                assert pkg.last_kernel() == kernel(cross), (what, pkg.last_kernel())
                assert_same(got, want, f"{what} shininess {k}")
        assert pkg.layout_info()["resident_bytes"] == copies  # no layout copy made
    # and another light is another frame on the same rays
    pkg.set_transfer_function(RAND256)
    pkg.set_light(None)
    want = frame()
    set_light(pkg, LIGHTS[1])
    got = frame()
    assert np.array_equal(got[2], want[2]), what
    pkg.set_light(None)
    pkg.set_transfer_function(None)
    return int((got[0] != want[0]).sum())


def test_identity_record_planes(pkg, gpu):
    """methods 1/2/3 from the statistics planes and 10/11/12/13 from their own"""
    import torch
    vol = volume(DIMS, 8, "f32")
    pkg.init_distribution(vol)
    pkg.bake_stats()
    pkg.set_query_range(0.0, THETA, 8)
    pkg.set_quantile(0.5)
    pkg.set_query_target(np.asarray(vol[8, 10, 12]), "emd")
    pkg.set_isovalue(THETA, 8)
    pkg.bake_weighted()
    pkg.bake_quantile()
    pkg.bake_distance()
    pkg.bake_crossing()
    differ = 0
    for method in (1, 2, 3, 10, 11, 12, 13):
        differ = max(differ, identity(
            pkg, lambda: render(pkg, torch, W, H, camera("C1"), method=method), method == 13,
            f"method {method}"))
    assert differ > 400


def test_identity_codec_planes(pkg, orc, gpu):
    """methods 4/5/6 from a codec volume's planes"""
    import torch
    cb, t, e = orc.synth_codec(22, 18, 14, 8, seed=8)
    pkg.init_codec(cb, t, e)
    pkg.bake_stats()
    for method in (4, 5, 6):
        identity(pkg, lambda: render(pkg, torch, W, H, camera("C1"), method=method), False,
                 f"codec method {method}")


def test_identity_gmm_planes(pkg, gpu):
    """render_gmm_baked methods 1, 2, 10, 11 and 13 with the records freed"""
    import torch
    bake_gmm_planes(pkg)
    try:
        pkg.free_gmm()  # the planes need no records
        for method in (1, 2, 10, 11, 13):
            identity(pkg, lambda: gmm_frame(pkg, torch, camera("C1"), method), method == 13,
                     f"GMM method {method}")
    finally:
        pkg.set_light(None)
        pkg.set_transfer_function(None)
        pkg.release_gmm_stats()


# ---- 4. rays end where they end without the light ----

def test_samples_per_pixel_are_the_unlit_frame_s(pkg, gpu):
    import torch
    rng = np.random.default_rng(2503)
    for dims, nb in ((DIMS, 8), (BAKE, 4)):
        upload_F_planes(pkg, dims, nb, "f32")
        pkg.set_transfer_function(RAND256)
        for cam in ("C0", "C1", "S"):
            for method, blend, cross in PLANES:
                pkg.set_light(None)
                want = render(pkg, torch, W, H, camera(cam), method=method)
                assert pkg.last_kernel() == (TF_CROSS if cross else TF_BLEND)
                assert_same(want, unlit(dims, nb, "f32", cam, W, H, "rand256", blend), "unlit")
                ka, kd, ks = (float(v) for v in rng.random(3) * 2)
                pkg.set_light(ka, kd, ks, 1 << int(rng.integers(0, 8)))
                got = render(pkg, torch, W, H, camera(cam), method=method)
                assert pkg.last_kernel() == kernel(cross)
                assert np.array_equal(got[2], want[2]), (dims, cam, method, pkg.light())
                assert np.array_equal(got[1][..., 3], want[1][..., 3]), "alpha is not lit"
                assert (got[0] != want[0]).sum() > 300


# ---- 5. inherited launch features ----

@pytest.mark.parametrize("method,blend,cross", PLANES)
def test_tile_list_with_padding_and_a_miss_tile(pkg, gpu, method, blend, cross):
    """test_gpu_crossing.py's list of the 70 x 50 frame: tiles that hit, a padding
    entry (its slot stays untouched), a tile of misses only and right-edge tiles"""
    import torch
    fw, fh = 70, 50
    light = LIGHTS[1]
    upload_F_planes(pkg, DIMS, 8, "f32")
    pkg.set_transfer_function(RAND256)
    set_light(pkg, light)
    ref8, reff, refn, _ = reference(DIMS, 8, "f32", "C1", fw, fh, "rand256", blend, light)
    tiles = [12, PAD, 24, 13, 15, 1]
    assert np.all(refn[48:50, 0:64] < 0), "tile 24 must be a miss tile"
    n = len(tiles)
    dl = torch.from_numpy(np.array(tiles, np.uint32).view(np.int32)).cuda()
    out = torch.full((n * 256,), SENTINEL, dtype=torch.int32, device="cuda")
    out_f = torch.full((n * 256 * 4,), -7.0, dtype=torch.float32, device="cuda")
    steps = torch.full((n * 256,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, fw, fh, camera("C1"), query_method=method, d_output_f=out_f,
                             d_steps=steps, d_tile_list=dl, n_tiles=n))
    torch.cuda.synchronize()
    assert pkg.last_kernel() == kernel(cross)
    g8 = out.cpu().numpy().view(np.uint32).reshape(n, 4, 64)
    gf = out_f.cpu().numpy().reshape(n, 4, 64, 4)
    gn = steps.cpu().numpy().reshape(n, 4, 64)
    for s, t in enumerate(tiles):
        if t == PAD:
            assert np.all(g8[s] == SENTINEL) and np.all(gn[s] == -2) and np.all(gf[s] == -7.0)
            continue
        x0, y0 = (t % 2) * 64, (t // 2) * 4
        for ly in range(4):
            for lx in range(64):
                x, y = x0 + lx, y0 + ly
                if x >= fw or y >= fh:  # outside the image: nothing written
                    assert g8[s, ly, lx] == SENTINEL and gn[s, ly, lx] == -2
                    assert np.all(gf[s, ly, lx] == -7.0)
                elif refn[y, x] < 0:    # a miss: 0 in list mode
                    assert g8[s, ly, lx] == 0 and gn[s, ly, lx] == -1
                else:
                    assert g8[s, ly, lx] == ref8[y, x] and gn[s, ly, lx] == refn[y, x]
                    assert np.array_equal(gf[s, ly, lx], reff[y, x])
    assert np.all(g8[2, :2] == 0) and np.all(gn[2, :2] == -1)  # the miss tile's rows 48, 49


@pytest.mark.parametrize("method,blend,cross", PLANES)
def test_render_kernel_partial_coverage(pkg, gpu, method, blend, cross):
    """a grid of 3 x 5 blocks of 16 x 4 threads covers 48 x 20 pixels of the 64 x 48
    image: those equal the reference, every other pixel keeps its sentinel"""
    import torch
    light = LIGHTS[2]
    upload_F_planes(pkg, DIMS, 8, "f32")
    pkg.set_transfer_function(RAMP2)
    set_light(pkg, light)
    pkg.copyInvViewMatrix(camera("C0"))
    out = torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda")
    pkg.render_kernel((3, 5, 1), (16, 4, 1), out, W, H, 0.05, 1.0, 0.0, 1.0, method, DIMS)
    torch.cuda.synchronize()
    assert pkg.last_kernel() == kernel(cross)
    got = out.cpu().numpy().view(np.uint32).reshape(H, W)
    ref8, _, refn, _ = reference(DIMS, 8, "f32", "C0", W, H, "ramp2", blend, light)
    want = np.full((H, W), SENTINEL, np.uint32)
    want[:20, :48] = np.where(refn[:20, :48] >= 0, ref8[:20, :48], SENTINEL)
    assert (refn[:20, :48] >= 0).any() and (refn[:20, :48] < 0).any()
    assert np.array_equal(got, want), int(np.sum(got != want))


# ---- 6. a seeded sweep of lights and tables ----

@pytest.mark.parametrize("seed", range(12))
def test_random_lights_and_tables(pkg, gpu, seed):
    """12 random lights (coefficients in [0, 2): colours beyond 1 among them; every
    exponent), tables of 1 to 256 random entries in [-0.5, 1.5), windows, densities and
    views on the BAKE plane, whose footprints the volume's edge clamps"""
    import torch
    rng = np.random.default_rng(2600 + seed)
    n = int(rng.choice([1, 2, 9, 64, 255, 256])) if seed % 4 else 256
    table = (rng.random((n, 4)) * 2 - 0.5).astype(np.float32)
    table[:, 3] = np.abs(table[:, 3])
    ka, kd, ks = (float(f) for f in (rng.random(3) * 2).astype(np.float32))
    k = seed % 8
    cam = ("C0", "C1", "S")[seed % 3]
    method, blend, cross = PLANES[(seed // 3) % 2]
    dtype = ("f32", "f16")[(seed // 6) % 2]
    kw = dict(density=float(rng.choice([0.05, 0.3, 1.0])), brightness=float(rng.choice([1.0, 1.5])),
              toff=float(rng.choice([0.0, 0.1])), tscale=float(rng.choice([1.0, 1.7, -1.0])))
    upload_F_planes(pkg, BAKE, 4, dtype)
    pkg.set_transfer_function(table)
    pkg.set_light(ka, kd, ks, 1 << k)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((W * H,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, W, H, camera(cam), query_method=method, density=kw["density"],
                             brightness=kw["brightness"], transfer_offset=kw["toff"],
                             transfer_scale=kw["tscale"], d_output_f=out_f, d_steps=steps))
    torch.cuda.synchronize()
    assert pkg.last_kernel() == kernel(cross)
    got = (out.cpu().numpy().view(np.uint32).reshape(H, W), out_f.cpu().numpy().reshape(H, W, 4),
           steps.cpu().numpy().reshape(H, W))
    want = ref_shading.render_plane(cdf(BAKE, 4, dtype), W, H, camera(cam), table, (ka, kd, ks, k),
                                    blend=BLENDS[blend], **kw)
    assert (want[2] >= 0).sum() > 1000
    assert_same(got, want, f"seed {seed}: n {n} light {(ka, kd, ks, k)} {cam} {method} {kw}")


@pytest.mark.parametrize("light", ((0.3, 0.5, 0.0, 5), (0.1, 1.2, -0.0, 7), (0.4, 0.9, 0.0, 1)),
                         ids=("k5", "minus-zero-k7", "k1"))
def test_lights_without_a_highlight(pkg, gpu, light):
    """ks = 0 (and -0, which the setter admits) with k > 0 on lights that are not the
    identity: the kernel takes spec = ks without the squarings, numpy computes ks * p"""
    import torch
    ka, kd, ks, k = light
    for dims, nb, cam in ((DIMS, 8, "C1"), (BAKE, 4, "S")):
        upload_F_planes(pkg, dims, nb, "f32")
        pkg.set_transfer_function(RAND256)
        pkg.set_light(ka, kd, ks, 1 << k)
        assert np.signbit(pkg.light()["specular"]) == np.signbit(ks)
        for method, blend, cross in PLANES:
            got = render(pkg, torch, W, H, camera(cam), method=method)
            assert pkg.last_kernel() == kernel(cross)
            want = ref_shading.render_plane(cdf(dims, nb, "f32"), W, H, camera(cam), RAND256, light,
                                            blend=BLENDS[blend])
            assert_same(got, want, f"{light} {dims} method {method}")
            base = unlit(dims, nb, "f32", cam, W, H, "rand256", blend)
            assert (want[0] != base[0]).sum() > 300


# ---- 7. lifetime and refusals ----

def test_lifetime(pkg, gpu):
    import torch
    light = LIGHTS[1]
    upload_F_planes(pkg, DIMS, 8, "f32")
    before = pkg.layout_info()["resident_bytes"]
    set_light(pkg, light)
    state = pkg.light()
    want = reference(DIMS, 8, "f32", "C1", W, H, None, "combine", light)[:3]
    assert_same(render(pkg, torch, W, H, camera("C1"), method=13), want, "first")
    # freeCudaBuffers frees the table's device copy and every plane; the light stays set
    pkg.freeCudaBuffers()
    assert pkg.light() == state
    assert pkg.crossing_info() == (None, 0)
    upload_F_planes(pkg, DIMS, 8, "f32")
    assert_same(render(pkg, torch, W, H, camera("C1"), method=13), want, "after freeCudaBuffers")
    # a new volume, vr_convert_f16 and the releases keep it too
    pkg.convert_f16()
    pkg.release_crossing()
    pkg.release_stats()
    assert pkg.light() == state
    pkg.bake_crossing()
    assert_same(render(pkg, torch, W, H, camera("C1"), method=13),
                reference(DIMS, 8, "f16", "C1", W, H, None, "combine", light)[:3],
                "after vr_convert_f16")
    assert pkg.layout_info()["resident_bytes"] == before


def test_refusals(pkg, orc, gpu):
    """with the light on nothing falls back to an unlit frame: what has no lit plane
    march is VR_ERR_UNSUPPORTED, and succeeds as before once the light is cleared"""
    import torch
    lib = pkg._lib
    pkg.init_distribution(volume(DIMS, 8, "f32"))
    pkg.set_query_range(0.0, THETA, 8)
    (wm, sg), _ = gmm_records("f32")
    pkg.init_gmm(wm, sg)
    out = torch.zeros(GW * GH, dtype=torch.int32, device="cuda")
    m = camera("C0")
    dg = pkg.make_desc(out, GW, GH, m, query_method=1, volume_size=(1, 1, 1))
    d1 = pkg.make_desc(out, W, H, m, query_method=1)

    # flexible blocks next to the record volume (methods 8/9/0)
    pkg.init_flex(orc.synth_flex(22, 6, 32, ntemplates=11, seed=5))
    pkg.dataProcessing()
    # the first slab of a two-slab chain of the resident GMM volume (its halo slice too)
    nz = wm.shape[0]
    z_lo, z_hi = pkg.slabs.slab_bounds(nz, 2, pkg.slabs.march_direction(m, GW, GH))[0]
    rays = torch.zeros((GW * GH, pkg.slabs.RAY_WORDS), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")

    def gmm_render(slab=False):
        out.zero_()
        rays.zero_()
        cnt.zero_()
        pkg.render_gmm(dg, pkg.gmm_slab(z_lo, z_hi, rays, cnt) if slab else None)
        torch.cuda.synchronize()
        r = rays.cpu().numpy()
        r = r[np.lexsort(r.T[::-1])]  # (the alive list is appended to in no fixed order)
        return np.concatenate([out.cpu().numpy().ravel(), cnt.cpu().numpy().ravel(), r.ravel()])

    def flex_render(method):
        fo = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        ff = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        fs = torch.full((W * H,), -2, dtype=torch.int32, device="cuda")
        pkg.render(pkg.make_desc(fo, W, H, camera("C1"), query_method=method,
                                 volume_size=(1, 1, 1), d_output_f=ff, d_steps=fs,
                                 transfer_scale={9: 1 / 255, 0: 1 / 4000, 8: 1.0}[method]))
        torch.cuda.synchronize()
        return (fo.cpu().numpy().view(np.uint32).reshape(H, W), ff.cpu().numpy().reshape(H, W, 4),
                fs.cpu().numpy().reshape(H, W))

    calls = {
        "method 1 per step": lambda: render(pkg, torch, W, H, m, method=1),
        "method 10 per step": lambda: render(pkg, torch, W, H, m, method=10),
        "method 7": lambda: render(pkg, torch, W, H, m, method=7),
        "method 8": lambda: flex_render(8),
        "method 9": lambda: flex_render(9),
        "method 0": lambda: flex_render(0),
        "render_gmm": gmm_render,
        "render_gmm, a slab": lambda: gmm_render(slab=True),
        "count_footprint": lambda: pkg.count_footprint(d1),
        "footprint_bytes": lambda: pkg.footprint_bytes(d1),
    }
    try:
        before = {k: f() for k, f in calls.items()}
        for method in (8, 9, 0):
            assert (before[f"method {method}"][2] > 0).sum() > 100, method
        assert before["render_gmm, a slab"][GW * GH] > 0  # rays handed to the next slab
        set_light(pkg, LIGHTS[0])
        calls_lit = dict(calls)
        calls_lit["render_gmm_baked, no plane"] = lambda: pkg.render_gmm_baked(dg)
        for k, f in calls_lit.items():
            with pytest.raises(pkg.VRError) as e:
                f()
            assert e.value.status == lib.VR_ERR_UNSUPPORTED, k
            msg = str(e.value)
            assert "light" in msg and "bake" in msg and "vr_set_light(NULL)" in msg, (k, msg)
        # with the plane resident: a 2-D table or a projection at the same time
        pkg.bake_weighted()
        render(pkg, torch, W, H, m, method=10)
        assert pkg.last_kernel() == kernel(False)
        pkg.set_transfer_function_2d(np.zeros((2, 2, 4), np.float32), 10)
        with pytest.raises(pkg.VRError) as e:
            render(pkg, torch, W, H, m, method=10)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
        assert "2-D transfer function" in str(e.value), str(e.value)
        pkg.set_transfer_function_2d(None)
        for mode in ("max", "min", "mean"):
            pkg.set_projection(mode)
            with pytest.raises(pkg.VRError) as e:
                render(pkg, torch, W, H, m, method=10)
            assert e.value.status == lib.VR_ERR_UNSUPPORTED
            assert "once per ray" in str(e.value), str(e.value)
        pkg.set_projection(None)
        pkg.release_weighted()
        pkg.set_query_range(0.0, THETA, 8)
        pkg.set_light(None)
        for k, f in calls.items():
            after = f()
            if isinstance(after, tuple):
                assert_same(after, before[k], k)
            else:
                assert np.array_equal(after, before[k]), k
    finally:
        pkg.set_light(None)
        pkg.set_projection(None)
        pkg.set_transfer_function_2d(None)
        pkg.free_gmm()
