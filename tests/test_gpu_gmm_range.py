"""GPU parity of the range probability of GMM volumes (query method 10:
k_march_gmm_range(_h), k_bake_gmm_range, vr_bake_gmm_range, vr_render_gmm_baked;
DESIGN.md section 18) through the C-ABI against the numpy restatement of
ref_gmm_range: per-step frames of fp32 and f16 volumes, the baked plane voxel by
voxel, frames from the plane, slab-wise bakes, a tile list, slab chains, and the
states.  The statistic is fixed float arithmetic with a table both sides read
and the plane march blends the same 8 floats with the same filter, so the bar is
bit identity: packed RGBA8, float RGBA and samples per pixel all exactly equal.

Volumes: 26 x 22 x 18 for the per-step frames (test_gpu_gmm_f16's), 37 x 11 x 9
for the plane (x crosses the brick aprons at 15 and 30 and is no multiple of the
32 / 16 / 8 voxels a wave bakes at K = 8 / 16 / 32; the odd y leaves half a
y-pair brick), and a hand-made 8 x 6 x 5 one of edge-case components."""
import ctypes
import functools

import numpy as np
import pytest

import ref_gmm_range as ref
from test_gpu_gmm_baked import plane_pitches, unbrick
from test_gpu_gmm_f16 import CAMS, Frame, _records, cam, check, same

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = float("inf")
BIG, DIMS = (26, 22, 18), (37, 11, 9)
W, H = 80, 64
RANGES = [(0.25, 0.75), (0.4, 0.5), (0.5, INF), (-INF, 0.3)]
M10 = 10


@pytest.fixture
def clean(pkg):
    """no planes, no range and no GMM volume in either slot, before and after"""
    def drop():
        pkg.clear_gmm_range()
        pkg.release_gmm_stats()
        for slot in (1, 0):
            pkg.gmm_select(slot)
            pkg.free_gmm()
    drop()
    yield
    drop()


@functools.lru_cache(maxsize=None)
def table(pkg):
    return pkg.gmm_phi_table()


def records(orc, dims, K, dtype):
    """(records to upload, the fp32 records the statistic is decoded from)"""
    wm, sg, hwm, hsg, wwm, wsg = _records(orc, dims, K, K)
    return ((hwm, hsg), (wwm, wsg)) if dtype == "f16" else ((wm, sg), (wm, sg))


@functools.lru_cache(maxsize=None)
def want_plane(orc, pkg, dims, K, dtype, rng):
    _, (wm, sg) = records(orc, dims, K, dtype)
    p = ref.range_stat(wm, sg, rng[0], rng[1], table(pkg))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def want_frame(orc, pkg, dims, K, dtype, rng, c, density):
    return ref.render_plane(want_plane(orc, pkg, dims, K, dtype, rng), W, H, cam(pkg, c),
                            density=density)


def per_step(pkg, torch, m, density=0.05, method=M10):
    f = Frame(pkg, torch, W, H, m, method, density)
    pkg.render_gmm(f.desc)
    torch.cuda.synchronize()
    return f.get()


def baked(pkg, torch, m, density=0.05, method=M10):
    f = Frame(pkg, torch, W, H, m, method, density)
    pkg.render_gmm_baked(f.desc)
    torch.cuda.synchronize()
    return f.get()


def read_plane(pkg):
    """the range plane as the device holds it: (dims, (1, plane_floats) float32, slices baked)"""
    import torch
    dims, ptr, n, nbaked = pkg.gmm_range_info()
    assert ptr, "no baked range plane"
    out = np.zeros(n, np.float32)
    torch.cuda.synchronize()
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr),
                         ctypes.c_size_t(out.nbytes), 2) == 0
    return dims, out.reshape(1, n), nbaked


def assert_plane(pkg, want, dims, what):
    got_dims, plane, nbaked = read_plane(pkg)
    assert tuple(got_dims) == tuple(dims) and nbaked == dims[2], (what, got_dims, nbaked)
    home, apron, ax, used = unbrick(plane, dims)
    bad = np.argwhere(home[0].view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: differs at (z, y, x) = {bad[:4].tolist()}"
    bad = np.argwhere(apron[0].view(np.uint32) != want[:, :, ax].view(np.uint32))
    assert bad.size == 0, f"{what}: apron differs at (z, y, k) = {bad[:4].tolist()}"
    assert not plane[:, ~used].any(), f"{what}: padding written"


# ---- per-step frames ----

@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_per_step_frames(pkg, orc, gpu, clean, K, dtype):
    """every camera with every range, both densities with every camera and every
    range (the density alternates along the 4 x 4 grid's diagonals)"""
    import torch
    (wm, sg), _ = records(orc, BIG, K, dtype)
    pkg.init_gmm(wm, sg)
    assert pkg.gmm_dtype() == dtype
    name = "k_march_gmm_range_h<" if dtype == "f16" else "k_march_gmm_range<"
    for i, c in enumerate(CAMS):
        for j, rng in enumerate(RANGES):
            density = (0.05, 0.6)[(i + j) % 2]
            pkg.set_gmm_range(*rng)
            got = per_step(pkg, torch, cam(pkg, c), density)
            kernel = pkg.last_kernel()
            assert kernel.startswith(name) and f"<B={K},M=10>" in kernel, kernel
            check(got, want_frame(orc, pkg, BIG, K, dtype, rng, c, density),
                  f"K={K} {dtype} {c} {rng} d={density}")


# ---- a hand-made volume of edge cases ----

def hand_made(dtype):
    """8 x 6 x 5 x 8 components drawn from: mu anywhere / exactly on lo / on hi;
    sigma ordinary / 0 (a Dirac) / so large that every z lies in the first segment /
    so small that every z clamps / (fp32) with a reciprocal that overflows; weight
    ordinary / 0.  Range [0.25, 0.75)."""
    rng = np.random.default_rng(8065)
    shape = (5, 6, 8, 8)
    w = rng.random(shape) + 0.05
    w[rng.random(shape) < 0.2] = 0.0
    w = w / np.maximum(w.sum(-1, keepdims=True), 1e-6)
    mu = rng.random(shape)
    pick = rng.random(shape)
    mu[pick < 0.15] = 0.25
    mu[pick > 0.85] = 0.75
    sg = 0.005 + 0.05 * rng.random(shape)
    kinds = [0.0, 1000.0, 1e-4] + ([1e-39] if dtype == "f32" else [])
    pick = rng.integers(0, 2 * len(kinds), shape)   # half stay ordinary
    for k, v in enumerate(kinds):
        sg[pick == k] = v
    sg[0, 0, 0, :] = 1000.0     # whole voxels of one kind, too
    sg[0, 0, 1, :] = 1e-4
    sg[0, 0, 2, :] = 0.0
    mu[0, 0, 2, :4] = 0.25
    mu[0, 0, 2, 4:] = 0.75
    t = np.float16 if dtype == "f16" else np.float32
    wm = np.stack([w, mu], -1).astype(t)
    sg = sg.astype(t)
    for k in kinds:
        assert (sg == t(k)).any()
    if dtype == "f32":
        with np.errstate(all="ignore"):
            assert np.isinf(f32(1) / sg[sg == f32(1e-39)]).all()
    return wm, sg


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_hand_made_volume(pkg, orc, gpu, clean, dtype):
    import torch
    dims, rng = (8, 6, 5), (0.25, 0.75)
    wm, sg = hand_made(dtype)
    tab = table(pkg)
    want = ref.range_stat(wm, sg, *rng, tab)
    assert np.isfinite(want).all() and np.unique(want).size > 100
    # the statistic's corner cases are really there
    # voxel (2, 0, 0): Diracs, four on lo (inside), four on hi (outside)
    assert want[0, 0, 2] == ref.tree_sum(
        _seq4(wm[0, 0, 2, :, 0].astype(f32) * f32([1, 1, 1, 1, 0, 0, 0, 0])))
    pkg.init_gmm(wm, sg)
    pkg.set_gmm_range(*rng)
    pkg.bake_gmm_range()
    assert_plane(pkg, want, dims, f"hand-made {dtype}")
    for c in ("C0", "C1"):
        m = cam(pkg, c)
        wf = ref.render_plane(want, W, H, m, density=0.3)
        check(per_step(pkg, torch, m, 0.3), wf, f"hand-made {dtype} {c} per step")
        check(baked(pkg, torch, m, 0.3), wf, f"hand-made {dtype} {c} baked")


def _seq4(t):
    """(8,) terms -> (2,) lane partials, four in order"""
    t = np.asarray(t, f32).reshape(2, 4)
    p = t[:, 0]
    for j in (1, 2, 3):
        p = p + t[:, j]
    return p


# ---- the plane ----

@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_plane_values(pkg, orc, gpu, clean, K, dtype):
    """every voxel of the plane, apron duplicates included, is the reference's
    statistic of its record bit for bit; nothing else is written; X = 37 leaves a
    row tail at every K; a re-bake gives the same values"""
    (wm, sg), _ = records(orc, DIMS, K, dtype)
    rng = RANGES[K // 16]
    assert pkg.gmm_range_info()[1] is None
    pkg.init_gmm(wm, sg)
    pkg.set_gmm_range(*rng)
    pkg.bake_gmm_range()
    sy, sz = plane_pitches(DIMS[0], DIMS[1])
    assert pkg.gmm_range_info()[2] == sz * DIMS[2]
    assert pkg.gmm_stats_info()[1] is None  # the mean / variance planes are not made
    want = want_plane(orc, pkg, DIMS, K, dtype, rng)
    assert_plane(pkg, want, DIMS, f"K={K} {dtype}")
    pkg.bake_gmm_range()
    assert_plane(pkg, want, DIMS, f"K={K} {dtype} rebaked")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_baked_frames(pkg, orc, gpu, clean, K, dtype):
    """a frame from the plane equals the reference and the per-step frame of the same
    device at all four cameras; a plane march renders it"""
    import torch
    (wm, sg), _ = records(orc, DIMS, K, dtype)
    rng = RANGES[0]
    pkg.init_gmm(wm, sg)
    pkg.set_gmm_range(*rng)
    pkg.bake_gmm_range()
    for i, c in enumerate(CAMS):
        density = (0.05, 0.6)[i % 2]
        m = cam(pkg, c)
        what = f"K={K} {dtype} {c} d={density}"
        got = baked(pkg, torch, m, density)
        kernel = pkg.last_kernel()
        assert "<B=1,M=0>" in kernel and kernel.startswith(("k_march_pipe", "k_march_seg")), kernel
        check(got, want_frame(orc, pkg, DIMS, K, dtype, rng, c, density), what)
        same(got, per_step(pkg, torch, m, density), what + ": per-step march")
        assert pkg.last_kernel().startswith("k_march_gmm_range")


def test_slab_wise_bake(pkg, orc, gpu, clean):
    """slices [5, 9), [0, 3), [2, 6) uploaded as separate volumes -- out of order,
    overlapping, z_base > 0 -- each baked and freed: the plane and a frame equal
    those of the volume baked at once, rendered with no GMM volume resident"""
    import torch
    K, rng = 16, RANGES[1]
    (wm, sg), _ = records(orc, DIMS, K, "f16")
    pkg.set_gmm_range(*rng)
    m = cam(pkg, "C1")
    f = Frame(pkg, torch, W, H, m, M10)
    slabs = [(5, 9), (0, 3), (2, 6)]
    seen = set()
    for i, (lo, hi) in enumerate(slabs):
        if i == len(slabs) - 1:
            assert pkg.gmm_range_info()[3] == len(seen) == 7
            with pytest.raises(pkg.VRError) as e:
                pkg.render_gmm_baked(f.desc)
            assert e.value.status == pkg._lib.VR_ERR_STATE
        pkg.init_gmm(wm[lo:hi], sg[lo:hi], DIMS, z_base=lo)
        pkg.bake_gmm_range()
        pkg.free_gmm()
        seen |= set(range(lo, hi))
        assert pkg.gmm_range_info()[3] == len(seen)
    with pytest.raises(pkg.VRError) as e:
        pkg.gmm_info()  # nothing resident
    assert e.value.status == pkg._lib.VR_ERR_STATE
    assert_plane(pkg, want_plane(orc, pkg, DIMS, K, "f16", rng), DIMS, "slab-wise")
    pkg.render_gmm_baked(f.desc)
    torch.cuda.synchronize()
    check(f.get(), want_frame(orc, pkg, DIMS, K, "f16", rng, "C1", 0.05), "slab-wise frame")


def test_tile_list(pkg, orc, gpu, clean):
    """a shuffled tile list of a 130 x 9 frame (3 x 3 tiles, ragged right and bottom)
    with one padding entry and one tile left out: every listed slot holds its tile
    of the whole frame from the plane, misses as 0"""
    import torch
    K, TW, TH = 16, 64, 4
    w, h = 130, 9
    (wm, sg), _ = records(orc, DIMS, K, "f32")
    pkg.init_gmm(wm, sg)
    pkg.set_gmm_range(0.25, 0.75)
    pkg.bake_gmm_range()
    pkg.free_gmm()
    m = cam(pkg, "C0")
    whole = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    pkg.render_gmm_baked(pkg.make_desc(whole, w, h, m, query_method=M10, volume_size=(1, 1, 1)))
    torch.cuda.synchronize()
    whole = whole.cpu().numpy().view(np.uint32).reshape(h, w)
    assert whole.any() and not whole.all()  # hits and misses
    want = ref.render_plane(want_plane(orc, pkg, DIMS, K, "f32", (0.25, 0.75)), w, h, m)["out"]
    assert np.array_equal(whole, want)
    order = np.random.default_rng(5).permutation(9)[:8].astype(np.uint32)  # one tile omitted
    tiles = np.insert(order, 3, 0xFFFFFFFF)
    fill = 0x5A5A5A5A
    packed = torch.full((tiles.size * 256,), fill, dtype=torch.int32, device="cuda")
    dl = torch.from_numpy(tiles.view(np.int32).copy()).cuda()
    pkg.render_gmm_baked(pkg.make_desc(packed, w, h, m, query_method=M10, volume_size=(1, 1, 1),
                                       d_tile_list=dl, n_tiles=tiles.size))
    torch.cuda.synchronize()
    assert "<B=1,M=0>" in pkg.last_kernel()
    got = packed.cpu().numpy().view(np.uint32).reshape(tiles.size, TH, TW)
    for slot, t in enumerate(tiles):
        exp = np.full((TH, TW), fill, np.uint32)  # outside the image, padding: untouched
        if t != 0xFFFFFFFF:
            x0, y0 = int(t % 3) * TW, int(t // 3) * TH
            part = whole[y0:y0 + TH, x0:x0 + TW]
            exp[:part.shape[0], :part.shape[1]] = part
        assert np.array_equal(got[slot], exp), f"slot {slot} (tile {t})"


# ---- slab chains ----

@pytest.mark.parametrize("nslabs,c,dtype", [(2, "C1", "f32"), (3, "C0", "f16")])
def test_slab_chain(pkg, orc, gpu, clean, nslabs, c, dtype):
    """each slab resident alone (its slices + halo; the two-slab chain keeps them in
    the two slots), the alive list carried on: the chain ends with no ray alive in
    the whole-volume frame"""
    import torch
    K, rng, density = 16, (0.25, 0.75), 0.2
    (wm, sg), _ = records(orc, BIG, K, dtype)
    m = cam(pkg, c)
    bounds = pkg.slabs.slab_bounds(BIG[2], nslabs, pkg.slabs.march_direction(m, W, H))
    pkg.set_gmm_range(*rng)
    f = Frame(pkg, torch, W, H, m, M10, density)
    bufs = [torch.zeros((W * H, pkg.slabs.RAY_WORDS), dtype=torch.int32, device="cuda")
            for _ in range(2)]
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    n_in, carried = 0, []
    for i, (z_lo, z_hi) in enumerate(bounds):
        zb, ns = pkg.slabs.resident_slices(z_lo, z_hi, BIG[2])
        pkg.gmm_select(i % 2 if nslabs == 2 else 0)
        pkg.init_gmm(wm[zb:zb + ns], sg[zb:zb + ns], BIG, z_base=zb)
        rin = bufs[(i + 1) % 2] if i else None
        s = pkg.gmm_slab(z_lo, z_hi, bufs[i % 2], cnt[0:1], d_rays_in=rin, n_rays_in=n_in)
        pkg.render_gmm(f.desc, s)
        torch.cuda.synchronize()
        assert pkg.last_kernel().startswith("k_march_gmm_range") and "M=10" in pkg.last_kernel()
        n_in = int(cnt[0].item())
        carried.append(n_in)
    assert carried[-1] == 0 and carried[0] > 0, carried
    check(f.get(), want_frame(orc, pkg, BIG, K, dtype, rng, c, density), f"{nslabs} slabs {c}")


# ---- states ----

def test_states_and_errors(pkg, orc, gpu, clean):
    import torch
    E = pkg._lib
    K = 16
    (wm, sg), _ = records(orc, DIMS, K, "f32")
    m = cam(pkg, "C1")
    f = Frame(pkg, torch, W, H, m, M10)
    pkg.init_gmm(wm, sg)
    before = [per_step(pkg, torch, m, method=q) for q in (1, 2)]
    for call in (pkg.render_gmm, pkg.render_gmm_baked, lambda d: pkg.bake_gmm_range()):
        with pytest.raises(pkg.VRError) as e:
            call(f.desc)  # no range (and no plane)
        assert e.value.status == E.VR_ERR_STATE
    pkg.set_gmm_range(0.25, 0.75)
    with pytest.raises(pkg.VRError) as e:
        pkg.gmm_count_footprint(f.desc)  # no counting instance of the range probability
    assert e.value.status == E.VR_ERR_UNSUPPORTED
    with pytest.raises(pkg.VRError) as e:
        pkg.render_gmm(Frame(pkg, torch, W, H, m, 3).desc)
    assert e.value.status == E.VR_ERR_UNSUPPORTED
    # methods 1 / 2 render what they rendered, with a range set and a range plane resident
    pkg.bake_gmm_range()
    pkg.bake_gmm_stats()
    for q in (1, 2):
        same(per_step(pkg, torch, m, method=q), before[q - 1], f"method {q} with a range set")
        assert pkg.last_kernel().startswith("k_march_gmm<")
        same(baked(pkg, torch, m, method=q), before[q - 1], f"baked method {q} beside the range plane")
    want = want_frame(orc, pkg, DIMS, K, "f32", (0.25, 0.75), "C1", 0.05)
    check(baked(pkg, torch, m), want, "baked range frame beside the stats planes")
    # the stats calls leave the range plane alone
    ptr = pkg.gmm_range_info()[1]
    pkg.release_gmm_stats()
    assert pkg.gmm_stats_info()[1] is None and pkg.gmm_range_info()[1] == ptr
    pkg.bake_gmm_stats()
    assert pkg.gmm_range_info()[1:] == (ptr, pkg.gmm_stats_info()[2], DIMS[2])
    check(baked(pkg, torch, m), want, "after release / bake of the stats planes")
    # the plane survives a change of slot, another volume and free_gmm
    pkg.gmm_select(1)
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_gmm_range()  # slot 1 is empty
    assert e.value.status == E.VR_ERR_STATE
    pkg.synthesize_gmm((16, 16, 16), 8)
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_gmm_range()  # other dims onto the existing plane
    assert e.value.status == E.VR_ERR_STATE
    pkg.free_gmm()
    pkg.gmm_select(0)
    pkg.free_gmm()
    assert_plane(pkg, want_plane(orc, pkg, DIMS, K, "f32", (0.25, 0.75)), DIMS, "after the refused bakes")
    check(baked(pkg, torch, m), want, "no records resident")
    # a new range and a cleared range drop the range plane, not the stats planes
    stats = pkg.gmm_stats_info()
    pkg.set_gmm_range(0.25, 0.75)  # even the same bounds
    assert pkg.gmm_range_info()[1:] == (None, 0, 0) and pkg.gmm_stats_info() == stats
    with pytest.raises(pkg.VRError) as e:
        pkg.render_gmm_baked(f.desc)
    assert e.value.status == E.VR_ERR_STATE
    pkg.init_gmm(wm, sg)
    pkg.bake_gmm_range()
    pkg.clear_gmm_range()
    assert pkg.gmm_range_info()[1] is None and pkg.gmm_stats_info() == stats
    same(baked(pkg, torch, m, method=1), before[0], "baked method 1 after the range went")
    pkg.set_gmm_range(0.4, 0.5)
    pkg.bake_gmm_range()
    pkg.release_gmm_range()
    assert pkg.gmm_range_info()[1] is None and pkg.gmm_range() == (float(f32(0.4)), 0.5)
    pkg.bake_gmm_range()
    pkg.freeCudaBuffers()
    assert pkg.gmm_range_info()[1] is None and pkg.gmm_stats_info()[1] is None
    with pytest.raises(pkg.VRError) as e:
        pkg.gmm_info()
    assert e.value.status == E.VR_ERR_STATE
