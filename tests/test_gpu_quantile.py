"""GPU checks of the quantile query (method 11: vr_quantile.hip, DESIGN.md
section 17).

The statistic -- prefix sums, a search for the bin the CDF crosses q in, one IEEE
division -- is float arithmetic in a fixed order which numpy float32 restates bit
for bit (tests/ref_quantile.py), so every comparison is exact: packed RGBA8, float
RGBA and samples per pixel are np.array_equal to the reference and planes are
compared as uint32, no tolerance and no pixel left out.  An f16 volume is
compared with the reference of its records widened to float32.
"""
import functools

import numpy as np
import pytest

import ref_quantile
import ref_weighted
from test_gpu_f16 import d2h
from test_gpu_parity import assert_parity
from test_gpu_weighted import expected_plane
from test_quantile import SPREAD, SPREAD_TSCALE

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
    pkg.set_quantile(None)
    pkg.set_bin_weights(None)
    yield
    pkg.set_quantile(None)
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
def reference(dims, nb, dtype, q, cam, w, h, tscale=1.0):
    """the numpy frame, computed once per case: (RGBA8, float RGBA, samples);
    q: a float, or (lo, hi) for the spread"""
    ref = ref_quantile.render(volume(dims, nb, dtype), q, w, h, camera(cam), tscale=tscale)
    for a in ref:
        a.setflags(write=False)
    return ref


def set_q(q):
    pkg = _state["pkg"]
    if isinstance(q, tuple):
        pkg.set_quantile_spread(*q)
    else:
        pkg.set_quantile(q)


def render11(torch, w, h, m, tscale=1.0):
    """one whole method-11 frame of the resident volume"""
    pkg = _state["pkg"]
    out = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(h * w * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((h * w,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, w, h, m, query_method=pkg.QUERY_QUANTILE, d_output_f=out_f,
                             d_steps=steps, transfer_scale=tscale))
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
    """every single-quantile instance at the median: fp32 B = 16, 32 and f16
    B = 32 gather in batches"""
    import torch
    pkg.init_distribution(volume(SMALL, nb, dtype))
    pkg.set_quantile(0.5)
    got = render11(torch, W, H, camera("C0"))
    assert pkg.volume_dtype() == dtype
    assert pkg.last_kernel() == f"k_march_quant<B={nb},M=11>"
    ref = reference(SMALL, nb, dtype, 0.5, "C0", W, H)
    assert (ref[2] > 0).any()
    assert_same(got, ref, f"x{nb} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", (8, 32))
def test_spread(pkg, gpu, nb, dtype):
    """the spread instances: the two-set loop (B = 8) and the batched one (B = 32)"""
    import torch
    pkg.init_distribution(volume(SMALL, nb, dtype))
    pkg.set_quantile_spread(*SPREAD)
    got = render11(torch, W, H, camera("C0"), SPREAD_TSCALE)
    assert pkg.last_kernel() == f"k_march_quant<B={nb},M=11>"
    ref = reference(SMALL, nb, dtype, SPREAD, "C0", W, H, SPREAD_TSCALE)
    hit = ref[2] > 0
    assert hit.any() and np.unique(ref[0][hit]).size > 1
    assert_same(got, ref, f"spread x{nb} {dtype}")
    # and it is not the single quantile's frame
    assert not np.array_equal(ref[1], reference(SMALL, nb, dtype, 0.5, "C0", W, H)[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cam,size", [("C0", (W, H)), ("C1", (W, H)), ("S", (W, H)),
                                      ("C1", (70, 50))])
def test_views_and_ragged_frame(pkg, gpu, cam, size, dtype):
    """row-aligned, oblique and side views all march the x rows; 70 x 50 is no
    multiple of the 64 x 4 tile"""
    import torch
    pkg.init_distribution(volume(DIMS, 8, dtype))
    pkg.set_quantile(0.5)
    got = render11(torch, *size, camera(cam))
    assert pkg.last_kernel() == "k_march_quant<B=8,M=11>"
    assert pkg.layout_info()["resident_bytes"] == 0  # no layout copy is used or made
    assert_same(got, reference(DIMS, 8, dtype, 0.5, cam, *size), f"{cam} {size} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_render_kernel_partial_coverage(pkg, gpu, dtype):
    """a grid of 3 x 5 blocks of 16 x 4 threads covers 48 x 20 pixels of the 64 x 48
    image: those equal the reference, every other pixel keeps its sentinel"""
    import torch
    pkg.init_distribution(volume(DIMS, 8, dtype))
    pkg.set_quantile(0.9)
    pkg.copyInvViewMatrix(camera("C0"))
    out = torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda")
    pkg.render_kernel((3, 5, 1), (16, 4, 1), out, W, H, 0.05, 1.0, 0.0, 1.0, pkg.QUERY_QUANTILE,
                      DIMS)
    torch.cuda.synchronize()
    assert pkg.last_kernel() == "k_march_quant<B=8,M=11>"
    got = out.cpu().numpy().view(np.uint32).reshape(H, W)
    ref8, _, refn = reference(DIMS, 8, dtype, 0.9, "C0", W, H)
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
    pkg.set_quantile(0.5)
    ref8, reff, refn = reference(DIMS, 8, dtype, 0.5, "C1", fw, fh)
    tiles = [12, PAD, 24, 13, 15, 1]
    assert np.all(refn[48:50, 0:64] < 0), "tile 24 must be a miss tile"
    assert (refn[24:28, 0:64] >= 0).any() and (refn[24:28, 64:70] >= 0).any()
    n = len(tiles)
    dl = torch.from_numpy(np.array(tiles, np.uint32).view(np.int32)).cuda()
    out = torch.full((n * 256,), SENTINEL, dtype=torch.int32, device="cuda")
    out_f = torch.full((n * 256 * 4,), -7.0, dtype=torch.float32, device="cuda")
    steps = torch.full((n * 256,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, fw, fh, camera("C1"), query_method=11, d_output_f=out_f,
                             d_steps=steps, d_tile_list=dl, n_tiles=n))
    torch.cuda.synchronize()
    assert pkg.last_kernel() == "k_march_quant<B=8,M=11>"
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
    pkg.set_quantile(0.5)
    for dtype in DTYPES:
        v = volume(DIMS, 8, dtype)
        t = torch.from_numpy(np.array(v)).cuda()
        pkg.init_distribution(t, adopt=True)
        assert pkg.volume_info()[2] == t.data_ptr() and pkg.volume_dtype() == dtype
        got = render11(torch, W, H, camera("C1"))
        assert_same(got, reference(DIMS, 8, dtype, 0.5, "C1", W, H), f"adopted {dtype}")
        pkg.bake_quantile()
        got = render11(torch, W, H, camera("C1"))
        assert_same(got, reference(DIMS, 8, dtype, 0.5, "C1", W, H), f"adopted baked {dtype}")
    tune.set("VR_PAD", "3,5")
    for dtype in DTYPES:
        pkg.init_distribution(volume(DIMS, 8, dtype))
        assert pkg.volume_layout() == (DIMS[0] + 3, (DIMS[0] + 3) * DIMS[1] + 5)
        got = render11(torch, W, H, camera("C0"))
        assert pkg.last_kernel() == "k_march_quant<B=8,M=11>"
        assert_same(got, reference(DIMS, 8, dtype, 0.5, "C0", W, H), f"pitched {dtype}")
        pkg.bake_quantile()
        got = render11(torch, W, H, camera("C0"))
        assert not pkg.last_kernel().startswith("k_march_quant")
        assert_same(got, reference(DIMS, 8, dtype, 0.5, "C0", W, H), f"pitched baked {dtype}")


@functools.lru_cache(maxsize=None)
def adversarial(nb, dtype):
    """37 x 5 x 3 records filled by hand: every third voxel takes the next of the
    special records below, the rest stay synthetic.  tiny: a bin that vanishes
    beside a bin of 1 -- 1e-40 (a float32 subnormal) or, for f16, 2^-24 (the
    smallest half subnormal); the other f16 values are exact in half or are
    rounded to half before the reference sees them."""
    nx, ny, nz = BAKE
    v = np.array(_state["orc"].synth_volume(nx, ny, nz, nb), dtype=np.float32)
    tiny = np.float32(2.0 ** -24 if dtype == "f16" else 1e-40)
    mid = nb // 2

    def only(i, mass):
        r = np.zeros(nb, np.float32)
        r[i] = mass
        return r

    def tie(i, j):  # c_i == tau exactly at q = 0.5, empty bins between i and j
        r = np.zeros(nb, np.float32)
        r[i] += 0.5
        r[j] += 0.5
        return r

    def negative(r):
        r[1] = -0.25
        return r

    alt = np.where(np.arange(nb) % 2 == 0, tiny, np.float32(1.0)).astype(np.float32)
    special = [
        lambda r: np.zeros(nb, np.float32),            # empty
        lambda r: only(0, 1.0),                        # all mass in the first bin,
        lambda r: only(mid, 2.5),                      # a middle bin,
        lambda r: only(nb - 1, 0.25),                  # the last bin
        lambda r: tie(0, nb - 1),                      # exact ties
        lambda r: tie(mid - 1, mid),
        lambda r: np.full(nb, 0.25, np.float32),       # c_i == tau at every bin edge
        lambda r: alt,                                 # tiny, 1, tiny, 1, ..
        lambda r: alt[::-1].copy(),                    # 1, tiny, ..
        lambda r: only(0, tiny) + only(nb - 1, 1.0),   # a tiny first bin, then the mass
        lambda r: only(0, tiny),                       # a tiny total
        lambda r: r * np.float32(1e-3),                # totals of 1e-3 and 3.7
        lambda r: r * np.float32(3.7),
        negative,                                      # a negative bin
    ]
    flat = v.reshape(-1, nb)
    for n, idx in enumerate(range(0, flat.shape[0], 3)):
        flat[idx] = special[n % len(special)](flat[idx].copy())
    if dtype == "f16":
        v = v.astype(np.float16)
        assert v[0, 0, 0].sum() == 0 and (v == np.float16(tiny)).any()
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", (4, 32))
def test_bake_adversarial_records(pkg, gpu, nb, dtype):
    """the statistic itself, voxel by voxel: the whole plane, aprons and zero
    padding included, against the numpy statistic at q = 0, 0.5, 1 and a spread"""
    v = adversarial(nb, dtype)
    wide = v.astype(np.float32)
    assert (wide.sum(-1) == 0).any() and (wide < 0).any()
    assert ((wide > 0) & (wide < 1e-6)).any()
    pkg.init_distribution(v)
    seen = set()
    for q in (0.0, 0.5, 1.0, SPREAD):
        set_q(q)
        assert pkg.quantile_info() == (None, 0)
        pkg.bake_quantile()
        ptr, n = pkg.quantile_info()
        stat = ref_quantile.quantile_stat(wide, q)
        assert np.all(np.isfinite(stat))
        want = expected_plane(stat)
        assert ptr and n == want.size
        got = d2h(ptr, n, np.float32)
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), (q, int(bad.sum()), got[bad][:4], want[bad][:4])
        seen.add(stat.tobytes())
    assert len(seen) == 4
    pkg.bake_quantile()  # baked already: nothing changes
    assert pkg.quantile_info() == (ptr, n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_baked_frames_equal_per_step_frames(pkg, gpu, dtype):
    import torch
    pkg.init_distribution(volume(BAKE, 4, dtype))
    for q, ts in ((0.5, 1.0), (SPREAD, SPREAD_TSCALE)):
        set_q(q)
        step = {}
        for cam in ("C0", "C1", "S"):
            step[cam] = render11(torch, W, H, camera(cam), ts)
            assert pkg.last_kernel() == "k_march_quant<B=4,M=11>"
            assert_same(step[cam], reference(BAKE, 4, dtype, q, cam, W, H, ts), f"step {cam}")
        pkg.bake_quantile()
        for cam in ("C0", "C1", "S"):
            got = render11(torch, W, H, camera(cam), ts)
            k = pkg.last_kernel()
            assert k.startswith("k_march_") and k.endswith("<B=1,M=0>") and "quant" not in k, k
            assert_same(got, step[cam], f"baked against per-step {cam}")
            assert_same(got, reference(BAKE, 4, dtype, q, cam, W, H, ts), f"baked {cam}")
        pkg.release_quantile()
        assert pkg.quantile_info() == (None, 0)


def test_state(pkg, gpu):
    import torch
    lib = pkg._lib
    m = camera("C0")
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    vol = volume(DIMS, 8, "f32")
    pkg.init_distribution(vol)
    d = pkg.make_desc(out, W, H, m, query_method=11)
    with pytest.raises(pkg.VRError) as e:  # no quantile
        pkg.render(d)
    assert e.value.status == lib.VR_ERR_STATE
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_quantile()
    assert e.value.status == lib.VR_ERR_STATE

    def baked():
        pkg.bake_quantile()
        assert pkg.quantile_info()[0]

    # every call that sets or clears the quantile drops the plane; the next frame is
    # per step and right for the new q
    pkg.set_quantile(0.9)
    baked()
    pkg.set_quantile(0.5)
    assert pkg.quantile_info() == (None, 0)
    got = render11(torch, W, H, m)
    assert pkg.last_kernel() == "k_march_quant<B=8,M=11>"
    assert_same(got, reference(DIMS, 8, "f32", 0.5, "C0", W, H), "after a change of q")
    baked()
    pkg.set_quantile_spread(*SPREAD)
    assert pkg.quantile_info() == (None, 0)
    got = render11(torch, W, H, m, SPREAD_TSCALE)
    assert_same(got, reference(DIMS, 8, "f32", SPREAD, "C0", W, H, SPREAD_TSCALE), "spread")
    baked()
    got = render11(torch, W, H, m, SPREAD_TSCALE)
    assert pkg.last_kernel().endswith("<B=1,M=0>")
    assert_same(got, reference(DIMS, 8, "f32", SPREAD, "C0", W, H, SPREAD_TSCALE), "spread baked")
    pkg.set_quantile(None)
    assert pkg.quantile_info() == (None, 0)
    # vr_release_quantile, vr_release_stats, a new upload and vr_convert_f16 drop it
    pkg.set_quantile(0.5)
    for drop in (pkg.release_quantile, pkg.release_stats, lambda: pkg.init_distribution(vol),
                 pkg.convert_f16):
        baked()
        drop()
        assert pkg.quantile_info() == (None, 0)
    # (vr_convert_f16 ran last: the volume is f16 now, and the frame is its frame)
    assert pkg.volume_dtype() == "f16" and pkg.quantile() == (0.5, 0.5, False)
    got = render11(torch, W, H, m)
    assert pkg.last_kernel() == "k_march_quant<B=8,M=11>"
    assert_same(got, reference(DIMS, 8, "f16", 0.5, "C0", W, H), "after vr_convert_f16")
    # freeCudaBuffers drops the plane and keeps the quantile, the caller's
    baked()
    pkg.freeCudaBuffers()
    assert pkg.quantile_info() == (None, 0)
    assert pkg.quantile() == (0.5, 0.5, False)
    # the weighted plane and the quantile plane are resident together, each
    # rendering its own frame; dropping one leaves the other
    pkg.init_distribution(vol)
    w = ref_weighted.seeded_weights(8)
    pkg.set_bin_weights(w)
    pkg.bake_weighted()
    baked()
    wp, qp = pkg.weighted_info(), pkg.quantile_info()
    assert wp[0] and qp[0] and wp[0] != qp[0] and wp[1] == qp[1]
    got = render11(torch, W, H, m)
    assert pkg.last_kernel().endswith("<B=1,M=0>")
    assert_same(got, reference(DIMS, 8, "f32", 0.5, "C0", W, H), "quantile plane")
    out10 = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out10, W, H, m, query_method=10))
    torch.cuda.synchronize()
    assert pkg.last_kernel().endswith("<B=1,M=0>")
    assert np.array_equal(out10.cpu().numpy().view(np.uint32).reshape(H, W),
                          ref_weighted.render(vol, w, W, H, m)[0])
    pkg.set_quantile(0.9)
    assert pkg.quantile_info() == (None, 0) and pkg.weighted_info() == wp
    baked()
    pkg.set_bin_weights(None)
    assert pkg.weighted_info() == (None, 0) and pkg.quantile_info()[0]
    # no footprint count of the quantile march
    for call in (pkg.count_footprint, pkg.footprint_bytes):
        with pytest.raises(pkg.VRError) as e:
            call(d)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
    # a runtime-B fp32 volume
    pkg.init_distribution(_state["orc"].synth_volume(6, 5, 4, 6))
    for call in (lambda: pkg.render(pkg.make_desc(out, W, H, m, query_method=11)),
                 pkg.bake_quantile):
        with pytest.raises(pkg.VRError) as e:
            call()
        assert e.value.status == lib.VR_ERR_UNSUPPORTED


def test_other_methods_unchanged(pkg, orc, gpu):
    """method-1, method-3 and method-10 frames of the same volume after quantile
    frames, per step and baked: the same frames from the kernels that rendered
    them before any quantile was set"""
    import torch
    from test_gpu_parity import gpu_render
    vol = volume(DIMS, 8, "f32")
    m = camera("C1")
    w = ref_weighted.seeded_weights(8)
    pkg.set_bin_weights(w)
    before = {}
    for method in (1, 3, 10):
        gpu_render(pkg, vol if method == 1 else None, W, H, m, method, torch)
        before[method] = pkg.last_kernel()
    assert before[10] == "k_march_lin<B=8,M=10>"
    pkg.set_quantile(0.5)
    assert_same(render11(torch, W, H, m), reference(DIMS, 8, "f32", 0.5, "C1", W, H), "step")
    pkg.bake_quantile()
    assert_same(render11(torch, W, H, m), reference(DIMS, 8, "f32", 0.5, "C1", W, H), "baked")
    for method in (1, 3):
        got = gpu_render(pkg, None, W, H, m, method, torch)
        assert pkg.last_kernel() == before[method]
        ref = orc.render(vol, orc.make_params(W, H, m, query_method=method))[:3]
        assert_parity(got, ref, f"method {method} after quantile frames")
    got = gpu_render(pkg, None, W, H, m, 10, torch)
    assert pkg.last_kernel() == before[10]
    assert_same(got, ref_weighted.render(vol, w, W, H, m), "method 10 after quantile frames")
    assert pkg.stats_info()[0][0] is None    # the quantile plane is not a statistics plane
    assert pkg.weighted_info() == (None, 0)  # nor the weighted plane
