"""GPU checks of the distribution-distance query (method 12: vr_distance.hip,
DESIGN.md section 20).

The statistic -- a subtraction per bin, a running sum and an add or a max of
magnitudes -- is float arithmetic in a fixed order which numpy float32 restates bit
for bit (tests/ref_distance.py), so every comparison is exact: packed RGBA8, float
RGBA and samples per pixel are np.array_equal to the reference and planes are
compared as uint32, no tolerance and no pixel left out.  An f16 volume is
compared with the reference of its records widened to float32.  The reference
frames are test_distance.py's, which checks on the CPU that each has hit pixels
of more than one colour.
"""
import numpy as np
import pytest

import ref_distance
import ref_quantile
import ref_weighted
from test_distance import (BAKE, BINS, DIMS, DIST_TSCALE, GPU_FRAMES, H, METRICS, REGION, SMALL,
                           W, camera, reference, target, volume)
from test_gpu_f16 import d2h
from test_gpu_weighted import expected_plane

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f16")
SENTINEL = 0x5A5A5A5A
PAD = 0xFFFFFFFF


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    def clear():
        pkg.set_query_target(None)
        pkg.set_quantile(None)
        pkg.set_bin_weights(None)
    clear()
    yield
    clear()
    pkg.release_stats()
    pkg.clear_tuning()


def ref(*case):
    """test_distance.reference, for the frames its CPU test has checked only"""
    case = case + ("centre",) if len(case) == 8 else case
    assert case in GPU_FRAMES, case
    return reference(*case)


def render(pkg, torch, w, h, m, method=12):
    """one whole frame of the resident volume"""
    out = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(h * w * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((h * w,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, w, h, m, query_method=method, d_output_f=out_f, d_steps=steps,
                             transfer_scale=DIST_TSCALE))
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint32).reshape(h, w),
            out_f.cpu().numpy().reshape(h, w, 4), steps.cpu().numpy().reshape(h, w))


def assert_same(got, want, what):
    for name, g, r in zip(("RGBA8", "float RGBA", "samples per pixel"), got, want):
        assert g.shape == r.shape, f"{what}: {name} shape"
        assert np.array_equal(g, r), f"{what}: {int(np.sum(g != r))} {name} values differ"


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", BINS)
def test_every_instance(pkg, gpu, nb, dtype, metric):
    """every march instance: fp32 B = 16, 32 and f16 B = 32 gather in batches"""
    import torch
    pkg.init_distribution(volume(SMALL, nb, dtype))
    pkg.set_query_target(target(SMALL, nb, dtype), metric)
    got = render(pkg, torch, W, H, camera("C0"))
    assert pkg.volume_dtype() == dtype
    assert pkg.last_kernel() == f"k_march_dist<B={nb},M=12>"
    assert_same(got, ref(SMALL, nb, dtype, metric, False, "C0", W, H), f"x{nb} {dtype} {metric}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_similarity_on_and_off(pkg, gpu, metric, dtype):
    import torch
    pkg.init_distribution(volume(DIMS, 8, dtype))
    frames = {}
    for sim in (False, True):
        pkg.set_query_target(target(DIMS, 8, dtype), metric, similarity=sim)
        frames[sim] = render(pkg, torch, W, H, camera("C0"))
        assert pkg.last_kernel() == "k_march_dist<B=8,M=12>"
        assert_same(frames[sim], ref(DIMS, 8, dtype, metric, sim, "C0", W, H),
                    f"{metric} similarity {sim} {dtype}")
    assert not np.array_equal(frames[False][1], frames[True][1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cam,size", [("C0", (W, H)), ("C1", (W, H)), ("S", (W, H)),
                                      ("C1", (70, 50))])
def test_views_and_ragged_frame(pkg, gpu, cam, size, dtype):
    """row-aligned, oblique and side views all march the x rows; 70 x 50 is no
    multiple of the 64 x 4 tile"""
    import torch
    pkg.init_distribution(volume(DIMS, 8, dtype))
    pkg.set_query_target(target(DIMS, 8, dtype), "emd")
    got = render(pkg, torch, *size, camera(cam))
    assert pkg.last_kernel() == "k_march_dist<B=8,M=12>"
    assert pkg.layout_info()["resident_bytes"] == 0  # no layout copy is used or made
    assert_same(got, ref(DIMS, 8, dtype, "emd", False, cam, *size), f"{cam} {size} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_render_kernel_partial_coverage(pkg, gpu, dtype):
    """a grid of 3 x 5 blocks of 16 x 4 threads covers 48 x 20 pixels of the 64 x 48
    image: those equal the reference, every other pixel keeps its sentinel"""
    import torch
    pkg.init_distribution(volume(DIMS, 8, dtype))
    pkg.set_query_target(target(DIMS, 8, dtype), "ks")
    pkg.copyInvViewMatrix(camera("C0"))
    out = torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda")
    pkg.render_kernel((3, 5, 1), (16, 4, 1), out, W, H, 0.05, 1.0, 0.0, DIST_TSCALE,
                      pkg.QUERY_DISTANCE, DIMS)
    torch.cuda.synchronize()
    assert pkg.last_kernel() == "k_march_dist<B=8,M=12>"
    got = out.cpu().numpy().view(np.uint32).reshape(H, W)
    ref8, _, refn = ref(DIMS, 8, dtype, "ks", False, "C0", W, H)
    want = np.full((H, W), SENTINEL, np.uint32)
    # a miss leaves a full frame untouched (K:302-303)
    want[:20, :48] = np.where(refn[:20, :48] >= 0, ref8[:20, :48], SENTINEL)
    assert (refn[:20, :48] >= 0).any() and (refn[:20, :48] < 0).any()
    assert np.array_equal(got, want), int(np.sum(got != want))


@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_list_with_padding_and_a_miss_tile(pkg, gpu, dtype):
    """a tile list of the 70 x 50 frame (2 x 13 tiles): tiles that hit, a padding
    entry (its slot stays untouched), a tile of misses only (written as 0; its rows
    beyond y = 49 are not rendered) and right-edge tiles, not rendered beyond x = 69"""
    import torch
    fw, fh = 70, 50
    pkg.init_distribution(volume(DIMS, 8, dtype))
    pkg.set_query_target(target(DIMS, 8, dtype), "emd")
    ref8, reff, refn = ref(DIMS, 8, dtype, "emd", False, "C1", fw, fh)
    tiles = [12, PAD, 24, 13, 15, 1]
    assert np.all(refn[48:50, 0:64] < 0), "tile 24 must be a miss tile"
    assert (refn[24:28, 0:64] >= 0).any() and (refn[24:28, 64:70] >= 0).any()
    n = len(tiles)
    dl = torch.from_numpy(np.array(tiles, np.uint32).view(np.int32)).cuda()
    out = torch.full((n * 256,), SENTINEL, dtype=torch.int32, device="cuda")
    out_f = torch.full((n * 256 * 4,), -7.0, dtype=torch.float32, device="cuda")
    steps = torch.full((n * 256,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, fw, fh, camera("C1"), query_method=12, d_output_f=out_f,
                             d_steps=steps, d_tile_list=dl, n_tiles=n,
                             transfer_scale=DIST_TSCALE))
    torch.cuda.synchronize()
    assert pkg.last_kernel() == "k_march_dist<B=8,M=12>"
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
    volumes with padded rows and slices (P.sy, P.sz): frames, the plane and the
    region's mean, which has to honour the pitches"""
    import torch
    for dtype in DTYPES:
        v = volume(DIMS, 8, dtype)
        t = torch.from_numpy(np.array(v)).cuda()
        pkg.init_distribution(t, adopt=True)
        assert pkg.volume_info()[2] == t.data_ptr() and pkg.volume_dtype() == dtype
        pkg.set_query_target(target(DIMS, 8, dtype), "emd")
        got = render(pkg, torch, W, H, camera("C1"))
        assert pkg.last_kernel() == "k_march_dist<B=8,M=12>"
        assert_same(got, ref(DIMS, 8, dtype, "emd", False, "C1", W, H), f"adopted {dtype}")
        pkg.bake_distance()
        got = render(pkg, torch, W, H, camera("C1"))
        assert_same(got, ref(DIMS, 8, dtype, "emd", False, "C1", W, H), f"adopted baked {dtype}")
        pkg.set_query_target_region(*REGION)
        assert np.array_equal(pkg.query_target()[0].view(np.uint32),
                              target(DIMS, 8, dtype, "region").view(np.uint32))
    tune.set("VR_PAD", "3,5")
    for dtype in DTYPES:
        pkg.init_distribution(volume(DIMS, 8, dtype))
        assert pkg.volume_layout() == (DIMS[0] + 3, (DIMS[0] + 3) * DIMS[1] + 5)
        pkg.set_query_target(target(DIMS, 8, dtype), "emd")
        got = render(pkg, torch, W, H, camera("C1"))
        assert pkg.last_kernel() == "k_march_dist<B=8,M=12>"
        assert_same(got, ref(DIMS, 8, dtype, "emd", False, "C1", W, H), f"pitched {dtype}")
        pkg.bake_distance()
        got = render(pkg, torch, W, H, camera("C1"))
        assert not pkg.last_kernel().startswith("k_march_dist")
        assert_same(got, ref(DIMS, 8, dtype, "emd", False, "C1", W, H), f"pitched baked {dtype}")
        pkg.set_query_target_region(*REGION)
        assert np.array_equal(pkg.query_target()[0].view(np.uint32),
                              target(DIMS, 8, dtype, "region").view(np.uint32))


@pytest.mark.parametrize("cap", ("1", "3"))
def test_wg_per_cu_changes_no_pixel(pkg, gpu, tune, cap):
    """VR_WG_PER_CU asks for LDS the kernel does not use, to cap the workgroups per
    CU: a scheduling knob only"""
    import torch
    tune.set("VR_WG_PER_CU", cap)
    for dtype, nb, dims in (("f32", 8, DIMS), ("f16", 32, SMALL)):
        pkg.init_distribution(volume(dims, nb, dtype))
        metric = "l1" if dims == SMALL else "emd"
        pkg.set_query_target(target(dims, nb, dtype), metric)
        got = render(pkg, torch, W, H, camera("C0"))
        assert pkg.last_kernel() == f"k_march_dist<B={nb},M=12>"
        assert_same(got, ref(dims, nb, dtype, metric, False, "C0", W, H), f"cap {cap} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", (4, 32))
def test_bake_plane(pkg, gpu, nb, dtype):
    """the statistic itself, voxel by voxel: the whole plane, aprons and zero padding
    included, against the numpy statistic, for every metric and the similarity"""
    v = volume(BAKE, nb, dtype)
    wide = v.astype(np.float32)
    h = target(BAKE, nb, dtype)
    pkg.init_distribution(v)
    seen = set()
    for metric in METRICS:
        for sim in (False, True):
            pkg.set_query_target(h, metric, sim)
            assert pkg.distance_info() == (None, 0)
            pkg.bake_distance()
            ptr, n = pkg.distance_info()
            stat = ref_distance.distance_stat(wide, h, metric, sim)
            assert np.all(np.isfinite(stat))
            want = expected_plane(stat)
            assert ptr and n == want.size
            got = d2h(ptr, n, np.float32)
            bad = got.view(np.uint32) != want.view(np.uint32)
            assert not bad.any(), (metric, sim, int(bad.sum()), got[bad][:4], want[bad][:4])
            seen.add(stat.tobytes())
    assert len(seen) == 6
    pkg.bake_distance()  # baked already: nothing changes
    assert pkg.distance_info() == (ptr, n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_baked_frames_equal_per_step_frames(pkg, gpu, dtype):
    import torch
    pkg.init_distribution(volume(BAKE, 4, dtype))
    pkg.set_query_target(target(BAKE, 4, dtype), "ks")
    step = {}
    for cam in ("C0", "C1", "S"):
        step[cam] = render(pkg, torch, W, H, camera(cam))
        assert pkg.last_kernel() == "k_march_dist<B=4,M=12>"
        assert_same(step[cam], ref(BAKE, 4, dtype, "ks", False, cam, W, H), f"step {cam}")
    pkg.bake_distance()
    for cam in ("C0", "C1", "S"):
        got = render(pkg, torch, W, H, camera(cam))
        k = pkg.last_kernel()
        assert k.startswith("k_march_") and k.endswith("<B=1,M=0>") and "dist" not in k, k
        assert_same(got, step[cam], f"baked against per-step {cam}")
        assert_same(got, ref(BAKE, 4, dtype, "ks", False, cam, W, H), f"baked {cam}")
    pkg.release_distance()
    assert pkg.distance_info() == (None, 0)


def test_state(pkg, orc, gpu):
    import torch
    lib = pkg._lib
    m = camera("C0")
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    vol = volume(DIMS, 8, "f32")
    h = target(DIMS, 8, "f32")
    pkg.init_distribution(vol)
    d = pkg.make_desc(out, W, H, m, query_method=12, transfer_scale=DIST_TSCALE)
    for bad in (None, target(SMALL, 4, "f32")):  # no target; a target of another bin count
        pkg.set_query_target(bad)
        for call in (lambda: pkg.render(d), pkg.bake_distance):
            with pytest.raises(pkg.VRError) as e:
                call()
            assert e.value.status == lib.VR_ERR_STATE

    def baked():
        pkg.bake_distance()
        assert pkg.distance_info()[0]

    # every call that sets or clears the target drops the plane; the next frame is
    # per step and right for the new state
    pkg.set_query_target(h, "l1")
    baked()
    pkg.set_query_target(h, "emd")
    assert pkg.distance_info() == (None, 0)
    got = render(pkg, torch, W, H, m)
    assert pkg.last_kernel() == "k_march_dist<B=8,M=12>"
    assert_same(got, ref(DIMS, 8, "f32", "emd", False, "C0", W, H), "after a change of metric")
    baked()
    got = render(pkg, torch, W, H, m)
    assert pkg.last_kernel().endswith("<B=1,M=0>")
    assert_same(got, ref(DIMS, 8, "f32", "emd", False, "C0", W, H), "baked")
    pkg.set_query_target_region(*REGION, metric="l1", similarity=True)
    assert pkg.distance_info() == (None, 0)
    baked()
    pkg.set_query_target(None)
    assert pkg.distance_info() == (None, 0)
    # vr_release_distance, vr_release_stats, a new upload and vr_convert_f16 drop it
    pkg.set_query_target(h, "emd")
    for drop in (pkg.release_distance, pkg.release_stats, lambda: pkg.init_distribution(vol),
                 pkg.convert_f16):
        baked()
        drop()
        assert pkg.distance_info() == (None, 0)
    # (vr_convert_f16 ran last: the volume is f16 now; the target is still the fp32
    # volume's, so the frame is rendered against the f16 volume's own)
    got_h, got_metric, got_sim = pkg.query_target()
    assert pkg.volume_dtype() == "f16" and np.array_equal(got_h, h)
    assert (got_metric, got_sim) == ("emd", False)
    pkg.set_query_target(target(DIMS, 8, "f16"), "emd")
    got = render(pkg, torch, W, H, m)
    assert pkg.last_kernel() == "k_march_dist<B=8,M=12>"
    assert_same(got, ref(DIMS, 8, "f16", "emd", False, "C0", W, H), "after vr_convert_f16")
    # freeCudaBuffers drops the plane and keeps the target, the caller's
    baked()
    pkg.freeCudaBuffers()
    assert pkg.distance_info() == (None, 0)
    assert np.array_equal(pkg.query_target()[0], target(DIMS, 8, "f16"))
    # the weighted, quantile and distance planes are resident together, each
    # rendering its own frame; dropping one leaves the others
    pkg.init_distribution(vol)
    pkg.set_query_target(h, "emd")
    w = ref_weighted.seeded_weights(8)
    pkg.set_bin_weights(w)
    pkg.set_quantile(0.5)
    pkg.bake_weighted()
    pkg.bake_quantile()
    baked()
    wp, qp, dp = pkg.weighted_info(), pkg.quantile_info(), pkg.distance_info()
    assert wp[0] and qp[0] and dp[0] and len({wp[0], qp[0], dp[0]}) == 3
    assert wp[1] == qp[1] == dp[1]
    got = render(pkg, torch, W, H, m)
    assert pkg.last_kernel().endswith("<B=1,M=0>")
    assert_same(got, ref(DIMS, 8, "f32", "emd", False, "C0", W, H), "distance plane")
    pkg.render(pkg.make_desc(out, W, H, m, query_method=10))
    torch.cuda.synchronize()
    assert pkg.last_kernel().endswith("<B=1,M=0>")
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(H, W),
                          ref_weighted.render(vol, w, W, H, m)[0])
    pkg.render(pkg.make_desc(out, W, H, m, query_method=11))
    torch.cuda.synchronize()
    assert pkg.last_kernel().endswith("<B=1,M=0>")
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(H, W),
                          ref_quantile.render(vol, 0.5, W, H, m)[0])
    pkg.set_query_target(h, "ks")  # the distance plane goes, theirs survive
    assert pkg.distance_info() == (None, 0)
    assert pkg.weighted_info() == wp and pkg.quantile_info() == qp
    baked()
    pkg.set_bin_weights(None)      # and it survives theirs
    pkg.set_quantile(None)
    assert pkg.weighted_info() == (None, 0) and pkg.quantile_info() == (None, 0)
    assert pkg.distance_info()[0]
    pkg.release_weighted()
    pkg.release_quantile()
    assert pkg.distance_info()[0]
    # no footprint count of the distance march
    for call in (pkg.count_footprint, pkg.footprint_bytes):
        with pytest.raises(pkg.VRError) as e:
            call(d)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
    # a runtime-B fp32 volume
    pkg.init_distribution(orc.synth_volume(6, 5, 4, 6))
    with pytest.raises(pkg.VRError) as e:
        pkg.render(d)
    assert e.value.status == lib.VR_ERR_UNSUPPORTED


@pytest.mark.parametrize("dtype", DTYPES)
def test_region_target(pkg, gpu, dtype):
    """query by example: the region's mean equals the reference's bit for bit, and
    its frame is the frame of the same target set by value"""
    import torch
    lib = pkg._lib
    L = lib.load()
    pkg.init_distribution(volume(DIMS, 8, dtype))
    want = target(DIMS, 8, dtype, "region")
    pkg.set_query_target_region(*REGION, metric="l1", similarity=True)
    h, metric, sim = pkg.query_target()
    assert (metric, sim) == ("l1", True)
    assert np.array_equal(h.view(np.uint32), want.view(np.uint32)), (h, want)
    by_region = render(pkg, torch, W, H, camera("C0"))
    assert pkg.last_kernel() == "k_march_dist<B=8,M=12>"
    pkg.set_query_target(want, "l1", similarity=True)
    by_value = render(pkg, torch, W, H, camera("C0"))
    assert_same(by_region, by_value, f"region against value {dtype}")
    assert_same(by_region, ref(DIMS, 8, dtype, "l1", True, "C0", W, H, "region"),
                f"region {dtype}")
    # one voxel: its record; the whole last row of the volume
    nx, ny, nz = DIMS
    v = volume(DIMS, 8, dtype)
    pkg.set_query_target_region((nx - 1, ny - 1, nz - 1), (nx, ny, nz), metric="ks")
    assert np.array_equal(pkg.query_target()[0], v[-1, -1, -1].astype(np.float32))
    pkg.set_query_target_region((0, ny - 1, nz - 1), (nx, ny, nz))
    assert np.array_equal(pkg.query_target()[0].view(np.uint32),
                          ref_distance.region_mean(v, (0, ny - 1, nz - 1), (nx, ny, nz))
                          .view(np.uint32))
    # boxes that are empty, outside the volume or too large; a bad metric: the state stays
    pkg.set_query_target(want, "emd")
    for box in ((3, 3, 3, 3, 4, 4), (3, 3, 3, 4, 4, 3), (5, 3, 3, 4, 4, 4), (-1, 0, 0, 1, 1, 1),
                (0, 0, 0, nx + 1, 1, 1), (0, 0, 0, 1, ny + 1, 1), (0, 0, 0, 1, 1, nz + 1),
                (0, 0, 0, 17, 16, 16)):
        assert L.vr_set_query_target_region(*box, 0, 0) == lib.VR_ERR_ARG, box
    assert L.vr_set_query_target_region(0, 0, 0, 1, 1, 1, 3, 0) == lib.VR_ERR_ARG
    got = pkg.query_target()
    assert np.array_equal(got[0], want) and got[1:] == ("emd", False)
    assert L.vr_set_query_target_region(0, 0, 0, 16, 16, 16, 0, 0) == lib.VR_OK  # 4096 voxels
    L.vr_clear_error()


def test_l1_against_zero_is_method_10_with_halves(pkg, gpu):
    """a check that needs no reference: on an f16 volume L1 with h = 0 is
    0.5 * sum p_i with the halving last, method 10 with every weight 0.5 the same
    with the halving first; halving commutes with every rounding when no operand is
    subnormal, and a widened half never is"""
    import torch
    for nb, dims, cam in ((8, DIMS, "C1"), (32, SMALL, "C0")):
        pkg.init_distribution(volume(dims, nb, "f16"))
        pkg.set_query_target(np.zeros(nb, np.float32), "l1")
        pkg.set_bin_weights(np.full(nb, 0.5, np.float32))
        a = render(pkg, torch, W, H, camera(cam), method=12)
        assert pkg.last_kernel() == f"k_march_dist<B={nb},M=12>"
        b = render(pkg, torch, W, H, camera(cam), method=10)
        assert pkg.last_kernel() == f"k_march_lin<B={nb},M=10>"
        hit = a[2] > 0
        assert hit.any() and np.unique(a[0][hit]).size > 1
        assert_same(a, b, f"L1 against method 10, x{nb}")


def test_unsupported(pkg, orc, gpu):
    """no footprint count of method 12, and no GMM frame"""
    import torch
    lib = pkg._lib
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    pkg.init_distribution(volume(SMALL, 4, "f32"))
    pkg.set_query_target(target(SMALL, 4, "f32"))
    d = pkg.make_desc(out, W, H, camera("C0"), query_method=12)
    for call in (pkg.count_footprint, pkg.footprint_bytes):
        with pytest.raises(pkg.VRError) as e:
            call(d)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
    wm, sg = orc.synth_gmm(16, 14, 12, 16)
    pkg.init_gmm(wm, sg)
    try:
        dg = pkg.make_desc(out, W, H, camera("C0"), query_method=12, volume_size=(1, 1, 1))
        with pytest.raises(pkg.VRError) as e:
            pkg.render_gmm(dg)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
        pkg.bake_gmm_stats()
        with pytest.raises(pkg.VRError) as e:
            pkg.render_gmm_baked(dg)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
    finally:
        pkg.release_gmm_stats()
        pkg.free_gmm()
