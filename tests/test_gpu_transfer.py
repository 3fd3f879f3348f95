"""GPU checks of the user-defined transfer function (vr_transfer.hip, DESIGN.md
section 22).

The classifier is float arithmetic in a fixed order which numpy float32 restates
bit for bit (tests/ref_transfer.py), so every comparison is exact: packed RGBA8,
float RGBA and samples per pixel are np.array_equal, no tolerance and no pixel left
out.  Two references: the library's own frames under the built-in table (a table of
the reference's nine entries must reproduce them through the new kernel), and
test_transfer.py's numpy frames, which that file checks on the CPU.
"""
import numpy as np
import pytest

from test_crossing import BAKE, DIMS, H, THETA, W, camera, volume
from test_gpu_crossing import (GH, GW, PAD, SENTINEL, assert_same, gmm_records, render)
from test_transfer import N255, ONE, RAMP2, RAND256, TABLES, reference

pytestmark = pytest.mark.gpu

TF_BLEND = "k_march_plane_tf<B=1,M=0>"
TF_CROSS = "k_march_plane_tf<B=1,M=13>"
# the two planes of F the numpy frames are marched over: method 10's (weights of
# [0, THETA): the plane of F itself, blended) and method 13's (combined)
PLANES = ((10, "trilinear", TF_BLEND), (13, "combine", TF_CROSS))


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    def clear():
        pkg.set_transfer_function(None)
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


def upload_F_planes(pkg, dims, nb, dtype):
    """the records resident with the method-10 and the method-13 plane of F baked"""
    pkg.init_distribution(volume(dims, nb, dtype))
    pkg.set_query_range(0.0, THETA, nb)
    pkg.set_isovalue(THETA, nb)
    pkg.bake_weighted()
    pkg.bake_crossing()


def ref(dims, nb, dtype, cam, w, h, table, blend):
    return reference(dims, nb, dtype, cam, w, h, table, blend)[:3]


# ---- 1. identity: the reference's nine entries through the new kernel ----

def identity(pkg, frame, new_kernel, what):
    pkg.set_transfer_function(None)
    want = frame()
    old = pkg.last_kernel()
    assert "k_march_plane_tf" not in old, old
    pkg.set_transfer_function(pkg.REFERENCE_TF)
    copies = pkg.layout_info()["resident_bytes"]
    got = frame()
    assert pkg.last_kernel() == new_kernel, (what, pkg.last_kernel())
    assert pkg.layout_info()["resident_bytes"] == copies  # no layout copy made
    hit = want[2] >= 0
    assert hit.sum() > 100 and np.unique(want[0][hit]).size > 1, what
    assert_same(got, want, what)
    return old


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
    for cam in ("C0", "C1"):
        for method in (1, 2, 3, 10, 11, 12, 13):
            old = identity(pkg, lambda: render(pkg, torch, W, H, camera(cam), method=method),
                           TF_CROSS if method == 13 else TF_BLEND, f"method {method} {cam}")
            if method == 13:
                assert old == "k_march_cross_plane<B=1,M=13>"
            else:
                assert old.endswith("<B=1,M=0>"), old


def test_identity_codec_planes(pkg, orc, gpu):
    """methods 4/5/6 from a codec volume's planes"""
    import torch
    cb, t, e = orc.synth_codec(22, 18, 14, 8, seed=8)
    pkg.init_codec(cb, t, e)
    pkg.bake_stats()
    for cam in ("C0", "C1"):
        for method in (4, 5, 6):
            old = identity(pkg, lambda: render(pkg, torch, W, H, camera(cam), method=method),
                           TF_BLEND, f"codec method {method} {cam}")
            assert "B=1,M=0>" in old, old


def gmm_frame(pkg, torch, m, method):
    out = torch.zeros(GH * GW, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(GH * GW * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((GH * GW,), -2, dtype=torch.int32, device="cuda")
    pkg.render_gmm_baked(pkg.make_desc(out, GW, GH, m, query_method=method, volume_size=(1, 1, 1),
                                       d_output_f=out_f, d_steps=steps))
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint32).reshape(GH, GW),
            out_f.cpu().numpy().reshape(GH, GW, 4), steps.cpu().numpy().reshape(GH, GW))


def bake_gmm_planes(pkg):
    (wm, sg), _ = gmm_records("f32")
    pkg.init_gmm(wm, sg)
    pkg.set_gmm_range(-float("inf"), THETA)
    pkg.set_quantile(0.5)
    pkg.bake_gmm_stats()
    pkg.bake_gmm_range()
    pkg.bake_gmm_quantile()


def test_identity_gmm_planes(pkg, gpu):
    """render_gmm_baked methods 1, 2, 10, 11 and 13 of the K = 16 volume"""
    import torch
    bake_gmm_planes(pkg)
    try:
        pkg.free_gmm()  # the planes need no records
        for cam in ("C0", "C1"):
            for method in (1, 2, 10, 11, 13):
                identity(pkg, lambda: gmm_frame(pkg, torch, camera(cam), method),
                         TF_CROSS if method == 13 else TF_BLEND, f"GMM method {method} {cam}")
    finally:
        pkg.set_transfer_function(None)
        pkg.release_gmm_stats()


# ---- 2. against numpy ----

NUMPY_CASES = (
    [(DIMS, 8, dt, cam, w, h) for dt in ("f32", "f16")
     for cam, w, h in (("C0", W, H), ("C1", W, H), ("S", W, H), ("C1", 70, 50))]
    + [(BAKE, 4, "f32", cam, W, H) for cam in ("C0", "C1", "S")] + [(BAKE, 4, "f16", "C1", W, H)]
)


@pytest.mark.parametrize("case", NUMPY_CASES, ids=lambda c: "-".join(
    "x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c))
def test_against_numpy(pkg, gpu, case):
    """ramp2, rand256, the one-entry and the 255-entry table (some threads stage
    nothing) on the method-10 and the method-13 plane"""
    import torch
    dims, nb, dtype, cam, w, h = case
    upload_F_planes(pkg, dims, nb, dtype)
    for name in ("ramp2", "rand256", "one", "n255"):
        pkg.set_transfer_function(TABLES[name])
        for method, blend, kernel in PLANES:
            got = render(pkg, torch, w, h, camera(cam), method=method)
            assert pkg.last_kernel() == kernel
            assert_same(got, ref(dims, nb, dtype, cam, w, h, name, blend),
                        f"{name} method {method} {case}")
    assert pkg.layout_info()["resident_bytes"] == 0  # no layout copy is used or made


def test_transfer_offset_and_scale(pkg, gpu):
    """x = (sample - offset) * scale as in every other frame"""
    import torch
    import ref_crossing
    import ref_transfer
    from test_crossing import cdf
    upload_F_planes(pkg, DIMS, 8, "f32")
    pkg.set_transfer_function(RAND256)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    for method, blend in ((10, ref_crossing.trilinear), (13, ref_crossing.combine)):
        pkg.render(pkg.make_desc(out, W, H, camera("C1"), query_method=method, density=0.2,
                                 brightness=1.5, transfer_offset=0.1, transfer_scale=1.7))
        torch.cuda.synchronize()
        want = ref_transfer.render_plane(cdf(DIMS, 8, "f32"), W, H, camera("C1"), RAND256,
                                         blend=blend, density=0.2, brightness=1.5, toff=0.1,
                                         tscale=1.7)[0]
        assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(H, W), want), method


# ---- 3. both addressing modes ----

def test_wide_addressing_changes_no_pixel(pkg, gpu, tune):
    import torch
    for dims, nb, dtype in ((DIMS, 8, "f32"), (BAKE, 4, "f16")):
        upload_F_planes(pkg, dims, nb, dtype)
        pkg.set_transfer_function(RAND256)
        for method, blend, kernel in PLANES:
            tune.clear("VR_TF_WIDE")
            narrow = render(pkg, torch, W, H, camera("C1"), method=method)
            tune.set("VR_TF_WIDE", "1")
            wide = render(pkg, torch, W, H, camera("C1"), method=method)
            assert pkg.last_kernel() == kernel
            assert_same(wide, narrow, f"VR_TF_WIDE {dims} method {method}")
            assert_same(wide, ref(dims, nb, dtype, "C1", W, H, "rand256", blend), "wide")
        tune.clear("VR_TF_WIDE")


# ---- 4. inherited launch features ----

@pytest.mark.parametrize("method,blend,kernel", PLANES)
def test_tile_list_with_padding_and_a_miss_tile(pkg, gpu, method, blend, kernel):
    """test_gpu_crossing.py's list of the 70 x 50 frame: tiles that hit, a padding
    entry (its slot stays untouched: the workgroup leaves after the staging barrier),
    a tile of misses only and right-edge tiles"""
    import torch
    fw, fh = 70, 50
    upload_F_planes(pkg, DIMS, 8, "f32")
    pkg.set_transfer_function(RAND256)
    ref8, reff, refn = ref(DIMS, 8, "f32", "C1", fw, fh, "rand256", blend)
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
    assert pkg.last_kernel() == kernel
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
                elif refn[y, x] < 0:    # a miss: 0 in list mode
                    assert g8[s, ly, lx] == 0 and gn[s, ly, lx] == -1
                else:
                    assert g8[s, ly, lx] == ref8[y, x] and gn[s, ly, lx] == refn[y, x]
                    assert np.array_equal(gf[s, ly, lx], reff[y, x])
    assert np.all(g8[2, :2] == 0) and np.all(gn[2, :2] == -1)  # the miss tile's rows 48, 49


@pytest.mark.parametrize("method,blend,kernel", PLANES)
def test_render_kernel_partial_coverage(pkg, gpu, method, blend, kernel):
    """a grid of 3 x 5 blocks of 16 x 4 threads covers 48 x 20 pixels of the 64 x 48
    image: those equal the reference, every other pixel keeps its sentinel"""
    import torch
    upload_F_planes(pkg, DIMS, 8, "f32")
    pkg.set_transfer_function(RAMP2)
    pkg.copyInvViewMatrix(camera("C0"))
    out = torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda")
    pkg.render_kernel((3, 5, 1), (16, 4, 1), out, W, H, 0.05, 1.0, 0.0, 1.0, method, DIMS)
    torch.cuda.synchronize()
    assert pkg.last_kernel() == kernel
    got = out.cpu().numpy().view(np.uint32).reshape(H, W)
    ref8, _, refn = ref(DIMS, 8, "f32", "C0", W, H, "ramp2", blend)
    want = np.full((H, W), SENTINEL, np.uint32)
    want[:20, :48] = np.where(refn[:20, :48] >= 0, ref8[:20, :48], SENTINEL)
    assert (refn[:20, :48] >= 0).any() and (refn[:20, :48] < 0).any()
    assert np.array_equal(got, want), int(np.sum(got != want))


@pytest.mark.parametrize("cap", ("1", "3", "7"))
def test_wg_per_cu_changes_no_pixel(pkg, gpu, tune, cap):
    """the cap's LDS request, less the table's static 4 KiB: a scheduling knob only"""
    import torch
    tune.set("VR_WG_PER_CU", cap)
    upload_F_planes(pkg, DIMS, 8, "f32")
    pkg.set_transfer_function(RAND256)
    for method, blend, kernel in PLANES:
        got = render(pkg, torch, W, H, camera("C0"), method=method)
        assert pkg.last_kernel() == kernel
        assert_same(got, ref(DIMS, 8, "f32", "C0", W, H, "rand256", blend), f"cap {cap}")


# ---- 5. table changes ----

@pytest.mark.parametrize("own_stream", (False, True))
def test_table_changes_reach_the_device(pkg, gpu, own_stream):
    """A, B, A again: a stale device copy would repeat a frame"""
    import torch
    upload_F_planes(pkg, DIMS, 8, "f32")
    stream = torch.cuda.Stream() if own_stream else None
    try:
        pkg.set_stream(stream)
        frames = []
        for name in ("ramp2", "rand256", "ramp2", "n255", "one"):
            pkg.set_transfer_function(TABLES[name])
            with torch.cuda.stream(stream) if own_stream else torch.cuda.stream(None):
                frames.append((name, render(pkg, torch, W, H, camera("C1"), method=13)))
        for name, got in frames:
            assert_same(got, ref(DIMS, 8, "f32", "C1", W, H, name, "combine"), name)
        assert_same(frames[2][1], frames[0][1], "A again")
        assert not np.array_equal(frames[1][1][0], frames[0][1][0])
        # back on the default stream after frames on another one
        pkg.set_stream(None)
        pkg.set_transfer_function(RAND256)
        got = render(pkg, torch, W, H, camera("C1"), method=10)
        assert_same(got, ref(DIMS, 8, "f32", "C1", W, H, "rand256", "trilinear"), "default stream")
    finally:
        torch.cuda.synchronize()
        pkg.set_stream(None)


# ---- 6. lifetime ----

def test_lifetime(pkg, gpu):
    import torch
    upload_F_planes(pkg, DIMS, 8, "f32")
    planes = (pkg.weighted_info(), pkg.crossing_info())
    assert planes[0][0] and planes[1][0]
    before = pkg.layout_info()["resident_bytes"]
    pkg.set_transfer_function(RAND256)
    assert (pkg.weighted_info(), pkg.crossing_info()) == planes  # setting drops no plane
    want = ref(DIMS, 8, "f32", "C1", W, H, "rand256", "combine")
    assert_same(render(pkg, torch, W, H, camera("C1"), method=13), want, "first")
    pkg.set_transfer_function(N255)
    pkg.set_transfer_function(RAND256)
    assert (pkg.weighted_info(), pkg.crossing_info()) == planes
    assert pkg.layout_info()["resident_bytes"] == before
    # freeCudaBuffers frees the device copy and every plane; the table stays set and
    # is uploaded again for the next frame, of a new upload
    pkg.freeCudaBuffers()
    assert np.array_equal(pkg.transfer_function(), RAND256)
    assert pkg.crossing_info() == (None, 0)
    upload_F_planes(pkg, DIMS, 8, "f32")
    assert_same(render(pkg, torch, W, H, camera("C1"), method=13), want, "after freeCudaBuffers")
    # a new volume, vr_convert_f16 and the releases keep it too
    pkg.convert_f16()
    pkg.release_crossing()
    pkg.release_stats()
    assert np.array_equal(pkg.transfer_function(), RAND256)
    pkg.bake_crossing()
    assert_same(render(pkg, torch, W, H, camera("C1"), method=13),
                ref(DIMS, 8, "f16", "C1", W, H, "rand256", "combine"), "after vr_convert_f16")
    assert pkg.layout_info()["resident_bytes"] == before


# ---- 7. refusals ----

def test_refusals(pkg, orc, gpu):
    """with a table set nothing falls back to the built-in one: what has no plane
    march is VR_ERR_UNSUPPORTED, and succeeds as before once the table is cleared"""
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

    def gmm_render():
        out.zero_()
        pkg.render_gmm(dg)
        torch.cuda.synchronize()
        return out.cpu().numpy().copy()

    calls = {
        "method 1 per step": lambda: render(pkg, torch, W, H, m, method=1),
        "method 10 per step": lambda: render(pkg, torch, W, H, m, method=10),
        "method 7": lambda: render(pkg, torch, W, H, m, method=7),
        "render_gmm": gmm_render,
        "count_footprint": lambda: pkg.count_footprint(d1),
    }
    try:
        before = {k: f() for k, f in calls.items()}
        pkg.set_transfer_function(RAMP2)
        for k, f in calls.items():
            with pytest.raises(pkg.VRError) as e:
                f()
            assert e.value.status == lib.VR_ERR_UNSUPPORTED, k
            assert "custom transfer function" in str(e.value) and "bake" in str(e.value), k
        with pytest.raises(pkg.VRError) as e:  # baked statistics planes do not serve method 7
            pkg.bake_stats()
            render(pkg, torch, W, H, m, method=7)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
        pkg.release_stats()
        pkg.set_query_range(0.0, THETA, 8)
        pkg.set_transfer_function(None)
        for k, f in calls.items():
            after = f()
            if isinstance(after, tuple):
                assert_same(after, before[k], k)
            else:
                assert np.array_equal(after, before[k]), k
    finally:
        pkg.set_transfer_function(None)
        pkg.free_gmm()
