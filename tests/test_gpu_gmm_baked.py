"""GPU parity of baked GMM statistics (k_bake_gmm, vr_bake_gmm_stats,
vr_render_gmm_baked) through the C-ABI: the two planes hold
the oracle's per-voxel statistics bit for bit, a frame from the planes equals
the oracle's GMM render and the per-step march of the same device, planes baked
slab by slab or through GmmStream.bake equal the ones baked at once, tile lists,
and the states and errors.  The statistic's evaluation order is fixed and the
plane march blends the same 8 floats with the same filter, so the bar is bit
identity: packed RGBA8, float RGBA and samples per pixel all exactly equal.

The volume is 37 x 11 x 9: x crosses the brick aprons at 15 and 30 and is no
multiple of the 32 / 16 / 8 voxels a wave bakes at K = 8 / 16 / 32, and the odd y
leaves half a y-pair brick."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_gmm_f16 import CAMS, Frame, _records, cam, check, same

pytestmark = pytest.mark.gpu

DIMS = (37, 11, 9)
W, H = 80, 64


@pytest.fixture
def clean(pkg):
    """no planes and no GMM volume in either slot, before and after"""
    def drop():
        pkg.release_gmm_stats()
        for slot in (1, 0):
            pkg.gmm_select(slot)
            pkg.free_gmm()
    drop()
    yield
    drop()


def records(orc, K, dtype):
    """(records to upload, the fp32 records the statistics are decoded from)"""
    wm, sg, hwm, hsg, wwm, wsg = _records(orc, DIMS, K, K)
    return ((hwm, hsg), (wwm, wsg)) if dtype == "f16" else ((wm, sg), (wm, sg))


@functools.lru_cache(maxsize=None)
def want_planes(orc, K, dtype):
    """(2, Z, Y, X) float32: orc.gmm_stat of every voxel, methods 1 and 2"""
    _, (wm, sg) = records(orc, K, dtype)
    X, Y, Z = DIMS
    out = np.zeros((2, Z, Y, X), np.float32)
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                for method in (1, 2):
                    out[method - 1, z, y, x] = orc.gmm_stat(wm[z, y, x], sg[z, y, x], method)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_frame(orc, pkg, K, dtype, c, method, density):
    _, (wm, sg) = records(orc, K, dtype)
    p = orc.make_params(W, H, cam(pkg, c), query_method=method, density=density)
    return orc.render_gmm(wm, sg, DIMS, p)


def plane_pitches(nx, ny):
    """include/vr.h: floats per y-pair row of bricks and per z slice"""
    sy = ((nx - 1) // 15 + 1) * 32
    return sy, ((ny + 1) // 2) * sy


def read_planes(pkg):
    """both planes as the device holds them: (dims, (2, plane_floats) float32, slices baked)"""
    import torch
    dims, ptr, n, nbaked = pkg.gmm_stats_info()
    assert ptr, "no baked GMM planes"
    out = np.zeros(2 * n, np.float32)
    torch.cuda.synchronize()
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr),
                         ctypes.c_size_t(out.nbytes), 2) == 0
    return dims, out.reshape(2, n), nbaked


def unbrick(planes, dims):
    """the 16 x 2 x 1 bricks undone with the vr.h formula: (home (2, Z, Y, X), the
    apron duplicates of x = 15 k > 0 (2, Z, Y, n), their x, a mask of every float
    that holds a voxel)"""
    X, Y, Z = dims
    sy, sz = plane_pitches(X, Y)
    assert planes.shape[1] == sz * Z
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    home = z * sz + (y // 2) * sy + (y % 2) * 16 + (x // 15) * 32 + x % 15
    ax = np.arange(15, X, 15)
    apron = home[:, :, ax] - 32 + 15
    used = np.zeros(planes.shape[1], bool)
    used[home.reshape(-1)] = True
    assert not used[apron.reshape(-1)].any()  # an apron slot is nobody's home
    used[apron.reshape(-1)] = True
    return planes[:, home], planes[:, apron], ax, used


def assert_planes(pkg, want, what):
    dims, planes, nbaked = read_planes(pkg)
    assert tuple(dims) == DIMS and nbaked == DIMS[2], (what, dims, nbaked)
    home, apron, ax, used = unbrick(planes, DIMS)
    for k, name in enumerate(("mean", "16 x variance")):
        bad = np.argwhere(home[k].view(np.uint32) != want[k].view(np.uint32))
        assert bad.size == 0, f"{what}: {name} differs at (z, y, x) = {bad[:4].tolist()}"
        bad = np.argwhere(apron[k].view(np.uint32) != want[k][:, :, ax].view(np.uint32))
        assert bad.size == 0, f"{what}: {name} apron differs at (z, y, k) = {bad[:4].tolist()}"
    assert not planes[:, ~used].any(), f"{what}: padding written"


def baked_render(pkg, torch, m, method, density=0.05):
    f = Frame(pkg, torch, W, H, m, method, density)
    pkg.render_gmm_baked(f.desc)
    torch.cuda.synchronize()
    return f.get()


def per_step_render(pkg, torch, m, method, density=0.05):
    f = Frame(pkg, torch, W, H, m, method, density)
    pkg.render_gmm(f.desc)
    torch.cuda.synchronize()
    return f.get()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_plane_values(pkg, orc, gpu, clean, K, dtype):
    """every voxel of both planes, apron duplicates included, is orc.gmm_stat of its
    record (f16: of the widened record) bit for bit; nothing else is written"""
    (wm, sg), _ = records(orc, K, dtype)
    assert pkg.gmm_stats_info()[1] is None
    pkg.init_gmm(wm, sg)
    assert pkg.gmm_dtype() == dtype
    pkg.bake_gmm_stats()
    sy, sz = plane_pitches(DIMS[0], DIMS[1])
    assert pkg.gmm_stats_info()[2] == sz * DIMS[2]
    assert_planes(pkg, want_planes(orc, K, dtype), f"K={K} {dtype}")
    pkg.bake_gmm_stats()  # again: the same values
    assert_planes(pkg, want_planes(orc, K, dtype), f"K={K} {dtype} rebaked")


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_whole_frames(pkg, orc, gpu, clean, K, dtype, method):
    """a frame from the planes equals the oracle's GMM render and the per-step march
    on the same device, four cameras and two densities; a plane march renders it"""
    import torch
    (wm, sg), _ = records(orc, K, dtype)
    pkg.init_gmm(wm, sg)
    pkg.bake_gmm_stats()
    for c in CAMS:
        for density in (0.05, 0.6):
            m = cam(pkg, c)
            what = f"K={K} {dtype} m{method} {c} d={density}"
            got = baked_render(pkg, torch, m, method, density)
            kernel = pkg.last_kernel()
            assert "<B=1,M=0>" in kernel and kernel.startswith(("k_march_pipe", "k_march_seg")), kernel
            check(got, want_frame(orc, pkg, K, dtype, c, method, density), what)
            same(got, per_step_render(pkg, torch, m, method, density), what + ": per-step march")
            assert pkg.last_kernel().startswith("k_march_gmm")


def test_slab_wise_bake(pkg, orc, gpu, clean):
    """slices [5, 9), [0, 3), [2, 6) uploaded as separate volumes -- out of order,
    overlapping, z_base > 0 -- each baked and freed: the planes and a frame equal
    those of the volume baked at once, rendered with no GMM volume resident"""
    import torch
    K = 16
    (wm, sg), _ = records(orc, K, "f32")
    m = cam(pkg, "C1")
    f = Frame(pkg, torch, W, H, m, 2)
    slabs = [(5, 9), (0, 3), (2, 6)]
    seen = set()
    for i, (lo, hi) in enumerate(slabs):
        if i == len(slabs) - 1:
            assert pkg.gmm_stats_info()[3] == len(seen) == 7
            with pytest.raises(pkg.VRError) as e:
                pkg.render_gmm_baked(f.desc)
            assert e.value.status == pkg._lib.VR_ERR_STATE
        pkg.init_gmm(wm[lo:hi], sg[lo:hi], DIMS, z_base=lo)
        pkg.bake_gmm_stats()
        pkg.free_gmm()
        seen |= set(range(lo, hi))
        assert pkg.gmm_stats_info()[3] == len(seen)
    with pytest.raises(pkg.VRError) as e:
        pkg.gmm_info()  # nothing resident
    assert e.value.status == pkg._lib.VR_ERR_STATE
    assert_planes(pkg, want_planes(orc, K, "f32"), "slab-wise")
    pkg.render_gmm_baked(f.desc)
    torch.cuda.synchronize()
    check(f.get(), want_frame(orc, pkg, K, "f32", "C1", 2, 0.05), "slab-wise frame")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("S", [1, 4, 9])
def test_stream_bake(pkg, orc, gpu, clean, S, dtype):
    """GmmStream.bake over host tensors, every slice its own slab (1), an uneven last
    slab (4) and a single slab (9): the planes of the volume baked at once"""
    import torch
    K = 16
    (wm, sg), _ = records(orc, K, dtype)
    st = pkg.stream.GmmStream(torch.from_numpy(wm.copy()), torch.from_numpy(sg.copy()), S)
    s = torch.cuda.Stream()
    try:
        info = st.bake(s)
        torch.cuda.synchronize()
    finally:
        pkg.set_stream(None)
    assert info["slabs"] == -(-DIMS[2] // S)
    assert info["bytes_streamed"] == wm.nbytes + sg.nbytes
    with pytest.raises(pkg.VRError):
        pkg.gmm_info()  # the ring buffer's view is released
    assert_planes(pkg, want_planes(orc, K, dtype), f"streamed S={S} {dtype}")
    got = baked_render(pkg, torch, cam(pkg, "C0"), 1)
    check(got, want_frame(orc, pkg, K, dtype, "C0", 1, 0.05), f"streamed S={S} {dtype} frame")


def test_tile_list(pkg, orc, gpu, clean):
    """a shuffled tile list of a 130 x 9 frame (3 x 3 tiles, ragged right and bottom)
    with one padding entry and one tile left out: every listed slot holds its tile
    of the whole baked frame, misses as 0"""
    import torch
    K, TW, TH = 16, 64, 4
    w, h = 130, 9
    (wm, sg), _ = records(orc, K, "f32")
    pkg.init_gmm(wm, sg)
    pkg.bake_gmm_stats()
    pkg.free_gmm()
    m = cam(pkg, "C0")
    whole = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    pkg.render_gmm_baked(pkg.make_desc(whole, w, h, m, query_method=2, volume_size=(1, 1, 1)))
    torch.cuda.synchronize()
    whole = whole.cpu().numpy().view(np.uint32).reshape(h, w)
    assert whole.any() and not whole.all()  # hits and misses
    assert pkg.tiles.tiles_x(w) == 3 and pkg.tiles.tiles_y(h) == 3
    order = np.random.default_rng(5).permutation(9)[:8].astype(np.uint32)  # one tile omitted
    tiles = np.insert(order, 3, 0xFFFFFFFF)
    fill = 0x5A5A5A5A
    packed = torch.full((tiles.size * 256,), fill, dtype=torch.int32, device="cuda")
    dl = torch.from_numpy(tiles.view(np.int32).copy()).cuda()
    pkg.render_gmm_baked(pkg.make_desc(packed, w, h, m, query_method=2, volume_size=(1, 1, 1),
                                       d_tile_list=dl, n_tiles=tiles.size))
    torch.cuda.synchronize()
    assert "<B=1,M=0>" in pkg.last_kernel()
    got = packed.cpu().numpy().view(np.uint32).reshape(tiles.size, TH, TW)
    for slot, t in enumerate(tiles):
        want = np.full((TH, TW), fill, np.uint32)  # outside the image, padding: untouched
        if t != 0xFFFFFFFF:
            x0, y0 = int(t % 3) * TW, int(t // 3) * TH
            part = whole[y0:y0 + TH, x0:x0 + TW]
            want[:part.shape[0], :part.shape[1]] = part
        assert np.array_equal(got[slot], want), f"slot {slot} (tile {t})"


def test_states_and_errors(pkg, orc, gpu, clean):
    import torch
    E = pkg._lib
    K = 16
    (wm, sg), _ = records(orc, K, "f32")
    m = cam(pkg, "C1")
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_gmm_stats()  # no GMM volume in the slot
    assert e.value.status == E.VR_ERR_STATE
    f = Frame(pkg, torch, W, H, m, 1)
    with pytest.raises(pkg.VRError) as e:
        pkg.render_gmm_baked(f.desc)  # no planes
    assert e.value.status == E.VR_ERR_STATE
    pkg.init_gmm(wm, sg)
    before = per_step_render(pkg, torch, m, 2)
    pkg.bake_gmm_stats()
    # the per-step march is unchanged while planes exist
    same(per_step_render(pkg, torch, m, 2), before, "render_gmm with planes resident")
    assert pkg.last_kernel().startswith("k_march_gmm<")
    # the planes survive a change of slot and a volume in the other slot
    pkg.gmm_select(1)
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_gmm_stats()  # slot 1 is empty
    assert e.value.status == E.VR_ERR_STATE
    pkg.synthesize_gmm((16, 16, 16), 8)
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_gmm_stats()  # other dims onto existing planes
    assert e.value.status == E.VR_ERR_STATE
    pkg.free_gmm()
    pkg.gmm_select(0)
    assert_planes(pkg, want_planes(orc, K, "f32"), "after the refused bakes")
    for method in (3, 7):
        g = Frame(pkg, torch, W, H, m, method)
        with pytest.raises(pkg.VRError) as e:
            pkg.render_gmm_baked(g.desc)
        assert e.value.status == E.VR_ERR_UNSUPPORTED
    check(baked_render(pkg, torch, m, 1), want_frame(orc, pkg, K, "f32", "C1", 1, 0.05), "baked")
    pkg.release_gmm_stats()
    assert pkg.gmm_stats_info()[1:] == (None, 0, 0)
    with pytest.raises(pkg.VRError) as e:
        pkg.render_gmm_baked(f.desc)
    assert e.value.status == E.VR_ERR_STATE
    pkg.bake_gmm_stats()  # slot 0's records are still resident
    assert pkg.gmm_stats_info()[3] == DIMS[2]
    pkg.freeCudaBuffers()
    assert pkg.gmm_stats_info()[1] is None
    with pytest.raises(pkg.VRError) as e:
        pkg.render_gmm_baked(f.desc)
    assert e.value.status == E.VR_ERR_STATE


def test_histogram_and_gmm_planes_coexist(pkg, orc, gpu, clean):
    """a histogram volume's vr_bake_stats planes and the GMM planes, both resident:
    render() and render_gmm_baked() each keep rendering their own frames"""
    import torch
    K = 16
    (wm, sg), _ = records(orc, K, "f32")
    vol = orc.synth_volume(20, 18, 16, 8)
    m = cam(pkg, "C0")
    ref_h = orc.render(vol, orc.make_params(W, H, m, query_method=1), want_float=False,
                       want_steps=False)[0]
    ref_g = want_frame(orc, pkg, K, "f32", "C0", 1, 0.05)
    assert not np.array_equal(ref_h, ref_g["out"])
    try:
        pkg.init_distribution(vol)
        pkg.bake_stats()
        pkg.init_gmm(wm, sg)
        pkg.bake_gmm_stats()
        pkg.free_gmm()
        assert pkg.stats_info()[0][0] and pkg.gmm_stats_info()[1]
        for _ in range(2):
            out = torch.zeros(H * W, dtype=torch.int32, device="cuda")
            pkg.render(pkg.make_desc(out, W, H, m, query_method=1))
            torch.cuda.synchronize()
            assert "M=0" in pkg.last_kernel()
            assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(H, W), ref_h)
            check(baked_render(pkg, torch, m, 1), ref_g, "GMM planes beside histogram planes")
        pkg.release_gmm_stats()
        assert pkg.stats_info()[0][0]  # the histogram planes stay
        pkg.release_stats()
    finally:
        pkg.freeCudaBuffers()
