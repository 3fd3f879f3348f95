"""GPU checks of the weighted-bin query (method 10: vr_query.hip, DESIGN.md
section 16).

The statistic is s = sum w_i p_i in float with a separate multiply and add per
bin, which numpy float32 restates bit for bit (tests/ref_weighted.py), so every
comparison is exact: packed RGBA8, float RGBA and samples per pixel are
np.array_equal to the reference, no tolerance and no pixel left out.  An f16
volume is compared with the reference of its records widened to float32.
"""
import functools

import numpy as np
import pytest

import ref_weighted
from test_gpu_f16 import d2h
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

BINS = (1, 2, 4, 8, 16, 32)
DTYPES = ("f32", "f16")
SMALL = (12, 10, 9)
DIMS = (24, 20, 16)
BAKE = (37, 5, 3)   # x crosses two brick aprons (15, 30), y is odd
W, H = 64, 48
SENTINEL = 0x5A5A5A5A
PAD = 0xFFFFFFFF
_state = {}


@pytest.fixture(autouse=True)
def _handles(pkg, orc, gpu):
    _state["orc"], _state["pkg"] = orc, pkg
    pkg.set_bin_weights(None)
    yield
    pkg.set_bin_weights(None)
    pkg.release_stats()
    pkg.clear_tuning()


def camera(cam):
    pkg = _state["pkg"]
    if cam == "C0":
        return pkg.camera.single_test_inv_view()
    return pkg.camera.display_inv_view((0.0, 90.0) if cam == "S" else (30.0, 45.0))


@functools.lru_cache(maxsize=None)
def volume(dims, nb, dtype):
    v = _state["orc"].synth_volume(*dims, nb)
    if dtype == "f16":
        v = v.astype(np.float16)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def reference(dims, nb, dtype, wkey, cam, w, h):
    """the numpy frame, computed once per case: (RGBA8, float RGBA, samples)"""
    ref = ref_weighted.render(volume(dims, nb, dtype), np.array(wkey, np.float32), w, h,
                              camera(cam))
    for a in ref:
        a.setflags(write=False)
    return ref


def key(w):
    return tuple(float(x) for x in np.asarray(w, np.float32))


def render10(torch, w, h, m, out=None):
    """one whole method-10 frame of the resident volume"""
    pkg = _state["pkg"]
    out = torch.zeros(h * w, dtype=torch.int32, device="cuda") if out is None else out
    out_f = torch.zeros(h * w * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((h * w,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, w, h, m, query_method=pkg.QUERY_WEIGHTED, d_output_f=out_f,
                             d_steps=steps))
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint32).reshape(h, w),
            out_f.cpu().numpy().reshape(h, w, 4), steps.cpu().numpy().reshape(h, w))


def assert_same(got, ref, what):
    for name, g, r in zip(("RGBA8", "float RGBA", "samples per pixel"), got, ref):
        assert g.shape == r.shape, f"{what}: {name} shape"
        assert np.array_equal(g, r), f"{what}: {int(np.sum(g != r))} {name} values differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", BINS)
def test_every_bin_count(pkg, gpu, nb, dtype):
    """every instance: B = 32 (f16) and B = 16, 32 (fp32) gather in batches"""
    import torch
    w = pkg.range_weights(0.2, 0.7, nb)
    pkg.init_distribution(volume(SMALL, nb, dtype))
    pkg.set_bin_weights(w)
    got = render10(torch, W, H, camera("C0"))
    assert pkg.volume_dtype() == dtype
    assert pkg.last_kernel() == f"k_march_lin<B={nb},M=10>"
    ref = reference(SMALL, nb, dtype, key(w), "C0", W, H)
    assert (ref[2] > 0).any()
    assert_same(got, ref, f"x{nb} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cam,size", [("C0", (W, H)), ("C1", (W, H)), ("S", (W, H)),
                                      ("C1", (70, 50))])
def test_views_and_ragged_frame(pkg, gpu, cam, size, dtype):
    """row-aligned, oblique and side views all march the x rows; 70 x 50 is no
    multiple of the 64 x 4 tile"""
    import torch
    w = ref_weighted.seeded_weights(8)
    pkg.init_distribution(volume(DIMS, 8, dtype))
    pkg.set_bin_weights(w)
    got = render10(torch, *size, camera(cam))
    assert pkg.last_kernel() == "k_march_lin<B=8,M=10>"
    assert pkg.layout_info()["resident_bytes"] == 0  # no layout copy is used or made
    assert_same(got, reference(DIMS, 8, dtype, key(w), cam, *size), f"{cam} {size} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_render_kernel_partial_coverage(pkg, gpu, dtype):
    """a grid of 3 x 5 blocks of 16 x 4 threads covers 48 x 20 pixels of the 64 x 48
    image: those equal the reference, every other pixel keeps its sentinel"""
    import torch
    w = ref_weighted.seeded_weights(8)
    pkg.init_distribution(volume(DIMS, 8, dtype))
    pkg.set_bin_weights(w)
    pkg.copyInvViewMatrix(camera("C0"))
    out = torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda")
    pkg.render_kernel((3, 5, 1), (16, 4, 1), out, W, H, 0.05, 1.0, 0.0, 1.0, pkg.QUERY_WEIGHTED,
                      DIMS)
    torch.cuda.synchronize()
    assert pkg.last_kernel() == "k_march_lin<B=8,M=10>"
    got = out.cpu().numpy().view(np.uint32).reshape(H, W)
    ref8, _, refn = reference(DIMS, 8, dtype, key(w), "C0", W, H)
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
    w = ref_weighted.seeded_weights(8)
    pkg.init_distribution(volume(DIMS, 8, dtype))
    pkg.set_bin_weights(w)
    ref8, reff, refn = reference(DIMS, 8, dtype, key(w), "C1", fw, fh)
    tiles = [12, PAD, 24, 13, 15, 1]
    assert np.all(refn[48:50, 0:64] < 0), "tile 24 must be a miss tile"
    assert (refn[24:28, 0:64] >= 0).any() and (refn[24:28, 64:70] >= 0).any()
    n = len(tiles)
    dl = torch.from_numpy(np.array(tiles, np.uint32).view(np.int32)).cuda()
    out = torch.full((n * 256,), SENTINEL, dtype=torch.int32, device="cuda")
    out_f = torch.full((n * 256 * 4,), -7.0, dtype=torch.float32, device="cuda")
    steps = torch.full((n * 256,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, fw, fh, camera("C1"), query_method=10, d_output_f=out_f,
                             d_steps=steps, d_tile_list=dl, n_tiles=n))
    torch.cuda.synchronize()
    assert pkg.last_kernel() == "k_march_lin<B=8,M=10>"
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
    volumes with padded rows and slices (P.sy, P.sz)"""
    import torch
    w = ref_weighted.seeded_weights(8)
    pkg.set_bin_weights(w)
    for dtype in DTYPES:
        v = volume(DIMS, 8, dtype)
        t = torch.from_numpy(np.array(v)).cuda()
        pkg.init_distribution(t, adopt=True)
        assert pkg.volume_info()[2] == t.data_ptr() and pkg.volume_dtype() == dtype
        got = render10(torch, W, H, camera("C1"))
        assert_same(got, reference(DIMS, 8, dtype, key(w), "C1", W, H), f"adopted {dtype}")
        pkg.bake_weighted()
        got = render10(torch, W, H, camera("C1"))
        assert_same(got, reference(DIMS, 8, dtype, key(w), "C1", W, H), f"adopted baked {dtype}")
    tune.set("VR_PAD", "3,5")
    for dtype in DTYPES:
        pkg.init_distribution(volume(DIMS, 8, dtype))
        assert pkg.volume_layout() == (DIMS[0] + 3, (DIMS[0] + 3) * DIMS[1] + 5)
        got = render10(torch, W, H, camera("C0"))
        assert pkg.last_kernel() == "k_march_lin<B=8,M=10>"
        assert_same(got, reference(DIMS, 8, dtype, key(w), "C0", W, H), f"pitched {dtype}")
        pkg.bake_weighted()
        got = render10(torch, W, H, camera("C0"))
        assert not pkg.last_kernel().startswith("k_march_lin")
        assert_same(got, reference(DIMS, 8, dtype, key(w), "C0", W, H), f"pitched baked {dtype}")


def expected_plane(stat):
    """stat (nz, ny, nx) in the header's brick layout, apron copies included"""
    nz, ny, nx = stat.shape
    sy = ((nx - 1) // 15 + 1) * 32
    sz = ((ny + 1) // 2) * sy
    plane = np.zeros(sz * nz, np.float32)
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                row = z * sz + (y // 2) * sy + (y % 2) * 16
                plane[row + (x // 15) * 32 + x % 15] = stat[z, y, x]
                if x > 0 and x % 15 == 0:  # also at offset 15 of brick x / 15 - 1
                    plane[row + (x // 15 - 1) * 32 + 15] = stat[z, y, x]
    return plane


@pytest.mark.parametrize("dtype", DTYPES)
def test_bake(pkg, gpu, dtype):
    import torch
    v = volume(BAKE, 4, dtype)
    pkg.init_distribution(v)
    # products that are subnormal: weights of 1e-39 k
    tiny = (np.float32(1e-39) * np.arange(1, 5, dtype=np.float32)).astype(np.float32)
    assert np.all(tiny != 0) and np.all(tiny < np.finfo(np.float32).tiny)
    seeded = ref_weighted.seeded_weights(4)
    for w in (tiny, seeded):
        pkg.set_bin_weights(w)
        assert pkg.weighted_info() == (None, 0)
        pkg.bake_weighted()
        ptr, n = pkg.weighted_info()
        stat = ref_weighted.lin_stat(v.astype(np.float32), w)
        want = expected_plane(stat)
        assert ptr and n == want.size
        got = d2h(ptr, n, np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
        if w is tiny:
            assert np.count_nonzero(stat) > 0 and np.all(np.abs(stat) < np.finfo(np.float32).tiny)
    pkg.bake_weighted()  # baked already: nothing changes
    assert pkg.weighted_info() == (ptr, n)
    # frames: per step, then from the plane
    pkg.release_weighted()
    assert pkg.weighted_info() == (None, 0)
    step = {}
    for cam in ("C0", "C1", "S"):
        step[cam] = render10(torch, W, H, camera(cam))
        assert pkg.last_kernel() == "k_march_lin<B=4,M=10>"
        assert_same(step[cam], reference(BAKE, 4, dtype, key(seeded), cam, W, H), f"step {cam}")
    pkg.bake_weighted()
    for cam in ("C0", "C1", "S"):
        got = render10(torch, W, H, camera(cam))
        k = pkg.last_kernel()
        assert k.startswith("k_march_") and k.endswith("<B=1,M=0>") and "lin" not in k, k
        assert_same(got, step[cam], f"baked against per-step {cam}")
        assert_same(got, reference(BAKE, 4, dtype, key(seeded), cam, W, H), f"baked {cam}")


def test_state(pkg, gpu):
    import torch
    lib = pkg._lib
    m = camera("C0")
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    pkg.init_distribution(volume(DIMS, 8, "f32"))
    d = pkg.make_desc(out, W, H, m, query_method=10)
    with pytest.raises(pkg.VRError) as e:  # no weights
        pkg.render(d)
    assert e.value.status == lib.VR_ERR_STATE
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_weighted()
    assert e.value.status == lib.VR_ERR_STATE
    # a change of the weights drops the plane; the next frame is per step and
    # right for the new weights
    w1, w2 = pkg.range_weights(0.2, 0.7, 8), ref_weighted.seeded_weights(8)
    pkg.set_bin_weights(w1)
    pkg.bake_weighted()
    assert pkg.weighted_info()[0]
    pkg.set_bin_weights(w2)
    assert pkg.weighted_info() == (None, 0)
    got = render10(torch, W, H, m)
    assert pkg.last_kernel() == "k_march_lin<B=8,M=10>"
    assert_same(got, reference(DIMS, 8, "f32", key(w2), "C0", W, H), "after a weight change")
    # clearing them too
    pkg.bake_weighted()
    pkg.set_bin_weights(None)
    assert pkg.weighted_info() == (None, 0)
    # vr_release_stats, a new upload and freeCudaBuffers drop it
    pkg.set_bin_weights(w2)
    for drop in (pkg.release_stats, lambda: pkg.init_distribution(volume(DIMS, 8, "f32")),
                 pkg.convert_f16):
        pkg.bake_weighted()
        assert pkg.weighted_info()[0]
        drop()
        assert pkg.weighted_info() == (None, 0)
    # (vr_convert_f16 ran last: the volume is f16 now, and the frame is its frame)
    assert pkg.volume_dtype() == "f16"
    got = render10(torch, W, H, m)
    assert pkg.last_kernel() == "k_march_lin<B=8,M=10>"
    assert_same(got, reference(DIMS, 8, "f16", key(w2), "C0", W, H), "after vr_convert_f16")
    pkg.bake_weighted()
    pkg.freeCudaBuffers()
    assert pkg.weighted_info() == (None, 0)
    assert np.array_equal(pkg.bin_weights(), w2)  # the weights are the caller's, not the volume's
    # weights whose count is not the volume's bins
    pkg.init_distribution(volume(DIMS, 8, "f32"))
    pkg.set_bin_weights(np.ones(4, np.float32))
    for call in (lambda: pkg.render(d), pkg.bake_weighted):
        with pytest.raises(pkg.VRError) as e:
            call()
        assert e.value.status == lib.VR_ERR_STATE
    # no footprint count of the weighted march
    pkg.set_bin_weights(np.ones(8, np.float32))
    for call in (pkg.count_footprint, pkg.footprint_bytes):
        with pytest.raises(pkg.VRError) as e:
            call(d)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
    # a runtime-B fp32 volume
    pkg.init_distribution(_state["orc"].synth_volume(6, 5, 4, 6))
    with pytest.raises(pkg.VRError) as e:
        pkg.render(pkg.make_desc(out, W, H, m, query_method=10))
    assert e.value.status == lib.VR_ERR_UNSUPPORTED


def test_other_methods_unchanged(pkg, orc, gpu):
    """method-1 and method-3 frames of the same volume after weighted frames, per
    step and baked: the oracle's frames from the kernels that rendered them before
    any weights were set"""
    import torch
    from test_gpu_parity import gpu_render
    vol = volume(DIMS, 8, "f32")
    m = camera("C1")
    before = {}
    for method in (1, 3):
        gpu_render(pkg, vol if method == 1 else None, W, H, m, method, torch)
        before[method] = pkg.last_kernel()
    w = ref_weighted.seeded_weights(8)
    pkg.set_bin_weights(w)
    assert_same(render10(torch, W, H, m), reference(DIMS, 8, "f32", key(w), "C1", W, H), "step")
    pkg.bake_weighted()
    assert_same(render10(torch, W, H, m), reference(DIMS, 8, "f32", key(w), "C1", W, H), "baked")
    for method in (1, 3):
        got = gpu_render(pkg, None, W, H, m, method, torch)
        assert pkg.last_kernel() == before[method]
        ref = orc.render(vol, orc.make_params(W, H, m, query_method=method))[:3]
        assert_parity(got, ref, f"method {method} after weighted frames")
    assert pkg.stats_info()[0][0] is None  # the weighted plane is not a statistics plane
