"""GPU checks of the level-crossing query (method 13: vr_crossing.hip, DESIGN.md
section 21).

The sample -- method 10's multiply and add per bin for each corner's F, then seven
multiplications for each of the two products and two subtractions -- is float
arithmetic in a fixed order which numpy float32 restates bit for bit
(tests/ref_crossing.py), so every comparison is exact: packed RGBA8, float RGBA
and samples per pixel are np.array_equal to the reference and planes are compared
as uint32, no tolerance and no pixel left out.  An f16 volume is compared with
the reference of its records widened to float32.  The reference frames are
test_crossing.py's, which checks on the CPU that each has hit pixels of more than
one colour, samples in clamped cells and (B != 2) rays that end early.
"""
import functools

import numpy as np
import pytest

import ref_crossing
import ref_gmm_range
import ref_quantile
import ref_weighted
from test_crossing import (BAKE, BINS, DIMS, GPU_FRAMES, H, SMALL, THETA, W, camera, cdf,
                           reference, volume, weights)
from test_gpu_f16 import d2h
from test_gpu_weighted import expected_plane

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f16")
SENTINEL = 0x5A5A5A5A
PAD = 0xFFFFFFFF
PLANE_KERNEL = "k_march_cross_plane<B=1,M=13>"


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    def clear():
        pkg.set_crossing_weights(None)
        pkg.set_query_target(None)
        pkg.set_quantile(None)
        pkg.set_bin_weights(None)
    clear()
    yield
    clear()
    pkg.release_stats()
    pkg.clear_tuning()


def ref(*case):
    """test_crossing.reference's frame, for the frames its CPU test has checked only"""
    assert case in GPU_FRAMES, case
    return reference(*case)[:3]


def render(pkg, torch, w, h, m, method=13):
    """one whole frame of the resident volume"""
    out = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(h * w * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((h * w,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, w, h, m, query_method=method, d_output_f=out_f, d_steps=steps))
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint32).reshape(h, w),
            out_f.cpu().numpy().reshape(h, w, 4), steps.cpu().numpy().reshape(h, w))


def assert_same(got, want, what):
    for name, g, r in zip(("RGBA8", "float RGBA", "samples per pixel"), got, want):
        assert g.shape == r.shape, f"{what}: {name} shape"
        assert np.array_equal(g, r), f"{what}: {int(np.sum(g != r))} {name} values differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", BINS)
def test_every_instance(pkg, gpu, nb, dtype):
    """every march instance: fp32 B = 16, 32 and f16 B = 32 gather in batches"""
    import torch
    pkg.init_distribution(volume(SMALL, nb, dtype))
    pkg.set_isovalue(THETA, nb)
    got = render(pkg, torch, W, H, camera("C0"))
    assert pkg.volume_dtype() == dtype
    assert pkg.last_kernel() == f"k_march_cross<B={nb},M=13>"
    assert_same(got, ref(SMALL, nb, dtype, "C0", W, H), f"x{nb} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cam,size", [("C0", (W, H)), ("C1", (W, H)), ("S", (W, H)),
                                      ("C1", (70, 50))])
def test_views_and_ragged_frame(pkg, gpu, cam, size, dtype):
    """row-aligned, oblique and side views all march the x rows; 70 x 50 is no
    multiple of the 64 x 4 tile"""
    import torch
    pkg.init_distribution(volume(DIMS, 8, dtype))
    pkg.set_isovalue(THETA, 8)
    got = render(pkg, torch, *size, camera(cam))
    assert pkg.last_kernel() == "k_march_cross<B=8,M=13>"
    assert pkg.layout_info()["resident_bytes"] == 0  # no layout copy is used or made
    assert_same(got, ref(DIMS, 8, dtype, cam, *size), f"{cam} {size} {dtype}")


@pytest.mark.parametrize("baked", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
def test_render_kernel_partial_coverage(pkg, gpu, dtype, baked):
    """a grid of 3 x 5 blocks of 16 x 4 threads covers 48 x 20 pixels of the 64 x 48
    image: those equal the reference, every other pixel keeps its sentinel"""
    import torch
    pkg.init_distribution(volume(DIMS, 8, dtype))
    pkg.set_isovalue(THETA, 8)
    if baked:
        pkg.bake_crossing()
    pkg.copyInvViewMatrix(camera("C0"))
    out = torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda")
    pkg.render_kernel((3, 5, 1), (16, 4, 1), out, W, H, 0.05, 1.0, 0.0, 1.0, pkg.QUERY_CROSSING,
                      DIMS)
    torch.cuda.synchronize()
    assert pkg.last_kernel() == (PLANE_KERNEL if baked else "k_march_cross<B=8,M=13>")
    got = out.cpu().numpy().view(np.uint32).reshape(H, W)
    ref8, _, refn = ref(DIMS, 8, dtype, "C0", W, H)
    want = np.full((H, W), SENTINEL, np.uint32)
    # a miss leaves a full frame untouched (K:302-303)
    want[:20, :48] = np.where(refn[:20, :48] >= 0, ref8[:20, :48], SENTINEL)
    assert (refn[:20, :48] >= 0).any() and (refn[:20, :48] < 0).any()
    assert np.array_equal(got, want), int(np.sum(got != want))


@pytest.mark.parametrize("baked", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_list_with_padding_and_a_miss_tile(pkg, gpu, dtype, baked):
    """a tile list of the 70 x 50 frame (2 x 13 tiles): tiles that hit, a padding
    entry (its slot stays untouched), a tile of misses only (written as 0; its rows
    beyond y = 49 are not rendered) and right-edge tiles, not rendered beyond x = 69"""
    import torch
    fw, fh = 70, 50
    pkg.init_distribution(volume(DIMS, 8, dtype))
    pkg.set_isovalue(THETA, 8)
    if baked:
        pkg.bake_crossing()
    ref8, reff, refn = ref(DIMS, 8, dtype, "C1", fw, fh)
    tiles = [12, PAD, 24, 13, 15, 1]
    assert np.all(refn[48:50, 0:64] < 0), "tile 24 must be a miss tile"
    assert (refn[24:28, 0:64] >= 0).any() and (refn[24:28, 64:70] >= 0).any()
    n = len(tiles)
    dl = torch.from_numpy(np.array(tiles, np.uint32).view(np.int32)).cuda()
    out = torch.full((n * 256,), SENTINEL, dtype=torch.int32, device="cuda")
    out_f = torch.full((n * 256 * 4,), -7.0, dtype=torch.float32, device="cuda")
    steps = torch.full((n * 256,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, fw, fh, camera("C1"), query_method=13, d_output_f=out_f,
                             d_steps=steps, d_tile_list=dl, n_tiles=n))
    torch.cuda.synchronize()
    assert pkg.last_kernel() == (PLANE_KERNEL if baked else "k_march_cross<B=8,M=13>")
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


def test_adopted_and_pitched_volumes(pkg, gpu, tune):
    """caller-owned buffers used in place (where = 2), fp32 and f16, and owned
    volumes with padded rows and slices (P.sy, P.sz): per-step and baked frames"""
    import torch
    for dtype in DTYPES:
        v = volume(DIMS, 8, dtype)
        t = torch.from_numpy(np.array(v)).cuda()
        pkg.init_distribution(t, adopt=True)
        assert pkg.volume_info()[2] == t.data_ptr() and pkg.volume_dtype() == dtype
        pkg.set_isovalue(THETA, 8)
        got = render(pkg, torch, W, H, camera("C1"))
        assert pkg.last_kernel() == "k_march_cross<B=8,M=13>"
        assert_same(got, ref(DIMS, 8, dtype, "C1", W, H), f"adopted {dtype}")
        pkg.bake_crossing()
        got = render(pkg, torch, W, H, camera("C1"))
        assert pkg.last_kernel() == PLANE_KERNEL
        assert_same(got, ref(DIMS, 8, dtype, "C1", W, H), f"adopted baked {dtype}")
    tune.set("VR_PAD", "3,5")
    for dtype in DTYPES:
        pkg.init_distribution(volume(DIMS, 8, dtype))
        assert pkg.volume_layout() == (DIMS[0] + 3, (DIMS[0] + 3) * DIMS[1] + 5)
        pkg.set_isovalue(THETA, 8)
        got = render(pkg, torch, W, H, camera("C1"))
        assert pkg.last_kernel() == "k_march_cross<B=8,M=13>"
        assert_same(got, ref(DIMS, 8, dtype, "C1", W, H), f"pitched {dtype}")
        pkg.bake_crossing()
        got = render(pkg, torch, W, H, camera("C1"))
        assert pkg.last_kernel() == PLANE_KERNEL
        assert_same(got, ref(DIMS, 8, dtype, "C1", W, H), f"pitched baked {dtype}")


@pytest.mark.parametrize("cap", ("1", "3"))
def test_wg_per_cu_changes_no_pixel(pkg, gpu, tune, cap):
    """VR_WG_PER_CU asks for LDS the kernels do not use, to cap the workgroups per
    CU: a scheduling knob only, per step and on the plane"""
    import torch
    tune.set("VR_WG_PER_CU", cap)
    for dtype, nb, dims in (("f32", 8, DIMS), ("f16", 32, SMALL)):
        pkg.init_distribution(volume(dims, nb, dtype))
        pkg.set_isovalue(THETA, nb)
        got = render(pkg, torch, W, H, camera("C0"))
        assert pkg.last_kernel() == f"k_march_cross<B={nb},M=13>"
        assert_same(got, ref(dims, nb, dtype, "C0", W, H), f"cap {cap} {dtype}")
        pkg.bake_crossing()
        got = render(pkg, torch, W, H, camera("C0"))
        assert pkg.last_kernel() == PLANE_KERNEL
        assert_same(got, ref(dims, nb, dtype, "C0", W, H), f"cap {cap} {dtype} baked")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", (4, 32))
def test_bake_plane(pkg, gpu, nb, dtype):
    """F itself, voxel by voxel: the whole plane, aprons and zero padding included,
    against numpy's lin_stat.  BAKE is 37 wide: x = 15 and x = 30 are written to
    two brick aprons."""
    v = volume(BAKE, nb, dtype)
    pkg.init_distribution(v)
    seen = set()
    for w in (weights(nb), ref_weighted.seeded_weights(nb)):
        pkg.set_crossing_weights(w)
        assert pkg.crossing_info() == (None, 0)
        pkg.bake_crossing()
        ptr, n = pkg.crossing_info()
        stat = ref_weighted.lin_stat(v.astype(np.float32), w)
        assert np.all(np.isfinite(stat))
        want = expected_plane(stat)
        assert ptr and n == want.size
        got = d2h(ptr, n, np.float32)
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), (int(bad.sum()), got[bad][:4], want[bad][:4])
        seen.add(stat.tobytes())
    assert len(seen) == 2
    pkg.bake_crossing()  # baked already: nothing changes
    assert pkg.crossing_info() == (ptr, n)
    assert np.array_equal(stat, ref_crossing.cdf_plane(v, ref_weighted.seeded_weights(nb)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_baked_frames_equal_per_step_frames(pkg, gpu, dtype):
    import torch
    pkg.init_distribution(volume(BAKE, 4, dtype))
    pkg.set_isovalue(THETA, 4)
    step = {}
    for cam in ("C0", "C1", "S"):
        step[cam] = render(pkg, torch, W, H, camera(cam))
        assert pkg.last_kernel() == "k_march_cross<B=4,M=13>"
        assert_same(step[cam], ref(BAKE, 4, dtype, cam, W, H), f"step {cam}")
    pkg.bake_crossing()
    for cam in ("C0", "C1", "S"):
        got = render(pkg, torch, W, H, camera(cam))
        assert pkg.last_kernel() == PLANE_KERNEL
        assert pkg.layout_info()["resident_bytes"] == 0
        assert_same(got, step[cam], f"baked against per-step {cam}")
        assert_same(got, ref(BAKE, 4, dtype, cam, W, H), f"baked {cam}")
    pkg.release_crossing()
    assert pkg.crossing_info() == (None, 0)


def test_state(pkg, orc, gpu):
    import torch
    lib = pkg._lib
    m = camera("C0")
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    vol = volume(DIMS, 8, "f32")
    pkg.init_distribution(vol)
    d = pkg.make_desc(out, W, H, m, query_method=13)
    for bad in (None, weights(4)):  # no weights; weights of another bin count
        pkg.set_crossing_weights(bad)
        for call in (lambda: pkg.render(d), pkg.bake_crossing):
            with pytest.raises(pkg.VRError) as e:
                call()
            assert e.value.status == lib.VR_ERR_STATE

    def baked():
        pkg.bake_crossing()
        assert pkg.crossing_info()[0]

    # every call that sets or clears the crossing weights drops the plane; the next
    # frame is per step and right for the new state
    pkg.set_isovalue(0.7, 8)
    baked()
    pkg.set_isovalue(THETA, 8)
    assert pkg.crossing_info() == (None, 0)
    got = render(pkg, torch, W, H, m)
    assert pkg.last_kernel() == "k_march_cross<B=8,M=13>"
    assert_same(got, ref(DIMS, 8, "f32", "C0", W, H), "after a change of isovalue")
    baked()
    got = render(pkg, torch, W, H, m)
    assert pkg.last_kernel() == PLANE_KERNEL
    assert_same(got, ref(DIMS, 8, "f32", "C0", W, H), "baked")
    pkg.set_crossing_weights(weights(8))  # the same weights set again: dropped all the same
    assert pkg.crossing_info() == (None, 0)
    baked()
    pkg.set_crossing_weights(None)
    assert pkg.crossing_info() == (None, 0)
    # vr_release_crossing, vr_release_stats, a new upload and vr_convert_f16 drop it
    pkg.set_isovalue(THETA, 8)
    for drop in (pkg.release_crossing, pkg.release_stats, lambda: pkg.init_distribution(vol),
                 pkg.convert_f16):
        baked()
        drop()
        assert pkg.crossing_info() == (None, 0)
        assert np.array_equal(pkg.crossing_weights(), weights(8))  # the caller's: kept
    # (vr_convert_f16 ran last: the volume is f16 now)
    assert pkg.volume_dtype() == "f16"
    got = render(pkg, torch, W, H, m)
    assert pkg.last_kernel() == "k_march_cross<B=8,M=13>"
    assert_same(got, ref(DIMS, 8, "f16", "C0", W, H), "after vr_convert_f16")
    # freeCudaBuffers drops the plane and keeps the weights
    baked()
    pkg.freeCudaBuffers()
    assert pkg.crossing_info() == (None, 0)
    assert np.array_equal(pkg.crossing_weights(), weights(8))
    # the weighted, quantile, distance and crossing planes are resident together,
    # each rendering its own frame; dropping one leaves the others
    pkg.init_distribution(vol)
    w = ref_weighted.seeded_weights(8)
    h = np.asarray(vol[8, 10, 12]).astype(np.float32)
    pkg.set_bin_weights(w)
    pkg.set_quantile(0.5)
    pkg.set_query_target(h, "emd")
    pkg.bake_weighted()
    pkg.bake_quantile()
    pkg.bake_distance()
    baked()
    wp, qp, dp, xp = (pkg.weighted_info(), pkg.quantile_info(), pkg.distance_info(),
                      pkg.crossing_info())
    assert all(p[0] for p in (wp, qp, dp, xp)) and len({wp[0], qp[0], dp[0], xp[0]}) == 4
    assert wp[1] == qp[1] == dp[1] == xp[1]
    got = render(pkg, torch, W, H, m)
    assert pkg.last_kernel() == PLANE_KERNEL
    assert_same(got, ref(DIMS, 8, "f32", "C0", W, H), "crossing plane")
    import ref_distance
    for method, want in ((10, ref_weighted.render(vol, w, W, H, m)[0]),
                         (11, ref_quantile.render(vol, 0.5, W, H, m)[0]),
                         (12, ref_distance.render(vol, h, "emd", False, W, H, m)[0])):
        pkg.render(pkg.make_desc(out, W, H, m, query_method=method))
        torch.cuda.synchronize()
        assert pkg.last_kernel().endswith("<B=1,M=0>")
        assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(H, W), want), method
    pkg.set_isovalue(0.7, 8)  # the crossing plane goes, theirs survive
    assert pkg.crossing_info() == (None, 0)
    assert (pkg.weighted_info(), pkg.quantile_info(), pkg.distance_info()) == (wp, qp, dp)
    pkg.set_isovalue(THETA, 8)
    baked()
    pkg.set_bin_weights(None)      # and it survives theirs
    pkg.set_quantile(None)
    pkg.set_query_target(None)
    assert pkg.weighted_info() == (None, 0) and pkg.quantile_info() == (None, 0)
    assert pkg.distance_info() == (None, 0)
    assert pkg.crossing_info()[0]
    pkg.release_weighted()
    pkg.release_quantile()
    pkg.release_distance()
    assert pkg.crossing_info()[0]
    got = render(pkg, torch, W, H, m)
    assert pkg.last_kernel() == PLANE_KERNEL
    assert_same(got, ref(DIMS, 8, "f32", "C0", W, H), "crossing plane alone")


def test_unsupported(pkg, orc, gpu):
    """no footprint count of method 13, no march for other bin counts, no per-step
    GMM frame"""
    import torch
    lib = pkg._lib
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    pkg.init_distribution(volume(SMALL, 4, "f32"))
    pkg.set_isovalue(THETA, 4)
    d = pkg.make_desc(out, W, H, camera("C0"), query_method=13)
    for call in (pkg.count_footprint, pkg.footprint_bytes):
        with pytest.raises(pkg.VRError) as e:
            call(d)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
    # a runtime-B fp32 volume
    pkg.init_distribution(orc.synth_volume(6, 5, 4, 6))
    with pytest.raises(pkg.VRError) as e:
        pkg.render(d)
    assert e.value.status == lib.VR_ERR_UNSUPPORTED
    wm, sg = orc.synth_gmm(16, 14, 12, 16)
    pkg.init_gmm(wm, sg)
    try:
        dg = pkg.make_desc(out, W, H, camera("C0"), query_method=13, volume_size=(1, 1, 1))
        with pytest.raises(pkg.VRError) as e:
            pkg.render_gmm(dg)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
    finally:
        pkg.free_gmm()


def test_zero_weights_are_method_10_with_zero_weights(pkg, gpu):
    """a check that needs no reference: with every weight 0 each F is 0, the combine
    gives (1 - 0) - 1 = 0 and method 10 samples 0 too: every sample is transparent,
    every ray runs its full length, and the frames are identical"""
    import torch
    for nb, dims, dtype, cam in ((8, DIMS, "f32", "C1"), (32, SMALL, "f16", "C0")):
        pkg.init_distribution(volume(dims, nb, dtype))
        pkg.set_crossing_weights(np.zeros(nb, np.float32))
        pkg.set_bin_weights(np.zeros(nb, np.float32))
        a = render(pkg, torch, W, H, camera(cam), method=13)
        assert pkg.last_kernel() == f"k_march_cross<B={nb},M=13>"
        b = render(pkg, torch, W, H, camera(cam), method=10)
        assert pkg.last_kernel() == f"k_march_lin<B={nb},M=10>"
        hit = a[2] > 0
        assert hit.any() and np.unique(a[2][hit]).size > 1  # rays of several lengths
        assert not a[0][hit].any() and not a[1].any()       # all transparent
        assert_same(a, b, f"zero weights against method 10, x{nb}")
        pkg.bake_crossing()
        c = render(pkg, torch, W, H, camera(cam), method=13)
        assert pkg.last_kernel() == PLANE_KERNEL
        assert_same(c, a, f"zero weights, baked, x{nb}")


# ---- GMM volumes through the range plane ----

GMM_DIMS, GMM_K = (37, 11, 9), 16
GW, GH = 80, 64


@functools.lru_cache(maxsize=None)
def gmm_records(dtype):
    """(records to upload, the fp32 records F is decoded from)"""
    import __graft_entry__ as graft
    wm, sg = graft.load_oracle().synth_gmm(*GMM_DIMS, GMM_K)
    if dtype == "f16":
        wm, sg = wm.astype(np.float16), sg.astype(np.float16)
        return (wm, sg), (wm.astype(np.float32), sg.astype(np.float32))
    return (wm, sg), (wm, sg)


def gmm_frame(pkg, torch, m, call):
    out = torch.zeros(GH * GW, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(GH * GW * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((GH * GW,), -2, dtype=torch.int32, device="cuda")
    call(pkg.make_desc(out, GW, GH, m, query_method=13, volume_size=(1, 1, 1), d_output_f=out_f,
                       d_steps=steps))
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint32).reshape(GH, GW),
            out_f.cpu().numpy().reshape(GH, GW, 4), steps.cpu().numpy().reshape(GH, GW))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gmm_crossing_through_the_range_plane(pkg, gpu, dtype):
    """vr_set_gmm_range(-inf, theta) bakes the mixture's CDF at theta; method 13 of
    vr_render_gmm_baked marches that plane with the crossing combine"""
    import torch
    lib = pkg._lib
    (wm, sg), (fwm, fsg) = gmm_records(dtype)
    pkg.clear_gmm_range()
    pkg.init_gmm(wm, sg)
    try:
        # no range, then a range without its plane: VR_ERR_STATE
        for prepare in (lambda: None, lambda: pkg.set_gmm_range(-float("inf"), THETA)):
            prepare()
            with pytest.raises(pkg.VRError) as e:
                gmm_frame(pkg, torch, camera("C0"), pkg.render_gmm_baked)
            assert e.value.status == lib.VR_ERR_STATE
        with pytest.raises(pkg.VRError) as e:
            gmm_frame(pkg, torch, camera("C0"), pkg.render_gmm)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
        pkg.bake_gmm_range()
        F = ref_gmm_range.range_stat(fwm, fsg, -float("inf"), THETA, pkg.gmm_phi_table())
        for cam in ("C0", "C1"):
            want = ref_crossing.render_plane(F, GW, GH, camera(cam))
            hit = want[2] >= 0
            colours = np.unique(want[0][hit] & 0x00FFFFFF).size
            print(f"{dtype} {cam}: {int(hit.sum())} hit, {colours} colours")
            assert hit.sum() > 1000 and colours > 100
            got = gmm_frame(pkg, torch, camera(cam), pkg.render_gmm_baked)
            assert pkg.last_kernel() == PLANE_KERNEL
            assert_same(got, want, f"GMM {dtype} {cam}")
    finally:
        pkg.clear_gmm_range()
        pkg.release_gmm_stats()
        pkg.free_gmm()
