"""GPU parity of the quantile of GMM volumes (query method 11:
k_march_gmm_quant(_h), k_bake_gmm_quant, vr_bake_gmm_quantile, vr_render_gmm_baked;
DESIGN.md section 19) through the C-ABI against the numpy restatement of
ref_gmm_quantile: per-step frames of fp32 and f16 volumes, a hand-made volume of
edge cases, the baked plane voxel by voxel, frames from the plane, slab-wise
bakes, a tile list, slab chains, the three GMM plane sets side by side, and the
states.  The statistic is fixed float arithmetic with a table and a step count
both sides read, and the plane march blends the same 8 floats with the same
filter, so the bar is bit identity: packed RGBA8, float RGBA and samples per
pixel all exactly equal.

Volumes: 23 x 20 x 18 for the per-step frames and 23 x 11 x 9 for the plane (x
crosses the brick apron at 15 and is no multiple of the 32 / 16 / 8 voxels a wave
bakes at K = 8 / 16 / 32, so the last wave of a row is partial; the odd y leaves
half a y-pair brick), and a hand-made 8 x 6 x 5 one."""
import ctypes
import functools

import numpy as np
import pytest

import ref_gmm_quantile as ref
from ref_gmm_range import render_plane
from test_gpu_gmm_baked import plane_pitches, unbrick
from test_gpu_gmm_f16 import Frame, _records, check, same

pytestmark = pytest.mark.gpu

f32 = np.float32
BIG, DIMS = (23, 20, 18), (23, 11, 9)
W, H = 80, 64
M11 = 11
IQR = (0.25, 0.75)
QUERIES = [0.0, 0.5, 0.9, 1.0, IQR]
# C0, C1, the side view S, and C1 moved in until the frame's edges clip the volume
CAMS = ("C0", "C1", "S", "clip")


def cam(pkg, c):
    if c == "C0":
        return pkg.camera.single_test_inv_view()
    if c == "S":
        return pkg.camera.display_inv_view((0.0, 90.0))
    if c == "clip":
        return pkg.camera.display_inv_view((30.0, 45.0), (0.3, 0.2, -2.0))
    return pkg.camera.display_inv_view((30.0, 45.0))


def set_q(pkg, q):
    if isinstance(q, tuple):
        pkg.set_quantile_spread(*q)
    else:
        pkg.set_quantile(q)


@pytest.fixture
def clean(pkg):
    """no GMM planes, no quantile, no range and no GMM volume in either slot, before
    and after"""
    def drop():
        pkg.set_quantile(None)
        pkg.clear_gmm_range()
        pkg.release_gmm_stats()
        for slot in (1, 0):
            pkg.gmm_select(slot)
            pkg.free_gmm()
    drop()
    yield
    drop()


@functools.lru_cache(maxsize=None)
def consts(pkg):
    return pkg.gmm_phi_table(), pkg.gmm_quantile_steps()


def stat(pkg, wm, sg, q):
    tab, n = consts(pkg)
    if isinstance(q, tuple):
        return ref.quantile_stat(wm, sg, q[0], q[1], True, tab, n)
    return ref.quantile_stat(wm, sg, q, q, False, tab, n)


def records(orc, dims, K, dtype):
    """(records to upload, the fp32 records the statistic is decoded from)"""
    wm, sg, hwm, hsg, wwm, wsg = _records(orc, dims, K, K)
    return ((hwm, hsg), (wwm, wsg)) if dtype == "f16" else ((wm, sg), (wm, sg))


@functools.lru_cache(maxsize=None)
def want_plane(orc, pkg, dims, K, dtype, q):
    _, (wm, sg) = records(orc, dims, K, dtype)
    p = stat(pkg, wm, sg, q)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def want_frame(orc, pkg, dims, K, dtype, q, c, density):
    return render_plane(want_plane(orc, pkg, dims, K, dtype, q), W, H, cam(pkg, c),
                        density=density)


def per_step(pkg, torch, m, density=0.05, method=M11):
    f = Frame(pkg, torch, W, H, m, method, density)
    pkg.render_gmm(f.desc)
    torch.cuda.synchronize()
    return f.get()


def baked(pkg, torch, m, density=0.05, method=M11):
    f = Frame(pkg, torch, W, H, m, method, density)
    pkg.render_gmm_baked(f.desc)
    torch.cuda.synchronize()
    return f.get()


def read_plane(pkg):
    """the quantile plane as the device holds it: (dims, (1, plane_floats) float32, slices baked)"""
    import torch
    dims, ptr, n, nbaked = pkg.gmm_quantile_info()
    assert ptr, "no baked quantile plane"
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
    assert bad.size == 0, (f"{what}: differs at (z, y, x) = {bad[:4].tolist()}: "
                           f"{home[0][tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}")
    bad = np.argwhere(apron[0].view(np.uint32) != want[:, :, ax].view(np.uint32))
    assert bad.size == 0, f"{what}: apron differs at (z, y, k) = {bad[:4].tolist()}"
    assert not plane[:, ~used].any(), f"{what}: padding written"


# ---- per-step frames ----

@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_per_step_frames(pkg, orc, gpu, clean, K, dtype):
    """every camera with every query (q = 0, 0.5, 0.9, 1 and the spread), both
    densities with every camera and every query (the density alternates along the
    4 x 5 grid's diagonals)"""
    import torch
    (wm, sg), _ = records(orc, BIG, K, dtype)
    pkg.init_gmm(wm, sg)
    assert pkg.gmm_dtype() == dtype
    name = "k_march_gmm_quant_h<" if dtype == "f16" else "k_march_gmm_quant<"
    for i, c in enumerate(CAMS):
        for j, q in enumerate(QUERIES):
            density = (0.05, 0.6)[(i + j) % 2]
            set_q(pkg, q)
            got = per_step(pkg, torch, cam(pkg, c), density)
            kernel = pkg.last_kernel()
            assert kernel.startswith(name) and f"<B={K},M=11>" in kernel, kernel
            want = want_frame(orc, pkg, BIG, K, dtype, q, c, density)
            hit = want["out_n"] > 0
            assert hit.any() and np.unique(want["out"][hit]).size > 20
            check(got, want, f"K={K} {dtype} {c} q={q} d={density}")
    # the clipped view really is: rays hit on the frame's border
    n = want_frame(orc, pkg, BIG, K, dtype, 0.5, "clip", 0.6)["out_n"]
    assert (n[0] > 0).any() and (n[:, 0] > 0).any()


# ---- a hand-made volume of edge cases ----

def hand_made(dtype):
    """8 x 6 x 5 x 8 components drawn from: sigma ordinary / 0 (a Dirac) / (fp32) a
    subnormal whose reciprocal overflows; weight ordinary / 0; mu on a coarse grid,
    so components coincide and bisection midpoints land on means.  Whole voxels of
    one kind in row (y, z) = (0, 0); all values are exact in binary16."""
    rng = np.random.default_rng(8066)
    shape = (5, 6, 8, 8)
    t = np.float16 if dtype == "f16" else np.float32
    w = (rng.integers(1, 9, shape) / 16.0)
    w[rng.random(shape) < 0.25] = 0.0
    mu = rng.integers(0, 17, shape) / 16.0
    sg = rng.integers(1, 8, shape) / 64.0
    tiny = 1e-39 if dtype == "f32" else 0.0   # 1 / sigma of any nonzero binary16 is finite
    pick = rng.integers(0, 6, shape)
    sg[pick == 0] = 0.0
    sg[pick == 1] = tiny
    # x = 0: no positive weight at all
    w[0, 0, 0, :] = 0.0
    # x = 1: Diracs at 1/4, 1/2, 3/4: the first midpoint is the middle Dirac
    w[0, 0, 1, :] = [0.25, 0.5, 0.25, 0, 0, 0, 0, 0]
    mu[0, 0, 1, :3] = [0.25, 0.5, 0.75]
    sg[0, 0, 1, :] = 0.0
    # x = 2: two Gaussians of equal reach around a third whose mean is the first midpoint
    w[0, 0, 2, :] = [0.25, 0.5, 0.25, 0, 0, 0, 0, 0]
    mu[0, 0, 2, :3] = [0.25, 0.5, 0.75]
    sg[0, 0, 2, :3] = [1 / 32.0, 1 / 64.0, 1 / 32.0]
    # x = 3: eight identical components
    w[0, 0, 3, :], mu[0, 0, 3, :], sg[0, 0, 3, :] = 0.125, 0.375, 1 / 32.0
    # x = 4: a bracket of one point -- all sigma 0, one mu
    w[0, 0, 4, :], mu[0, 0, 4, :], sg[0, 0, 4, :] = 0.125, 0.625, 0.0
    # x = 5: the same with reciprocals that overflow (fp32) and zero weights between
    w[0, 0, 5, :] = [0.5, 0, 0.25, 0, 0, 0.25, 0, 0]
    mu[0, 0, 5, :], sg[0, 0, 5, :] = 0.625, tiny
    # x = 6: one live Gaussian among zero-weight Diracs far outside its support
    w[0, 0, 6, :] = [0, 0, 0, 0, 0, 1.0, 0, 0]
    mu[0, 0, 6, :] = [0, 1, 0, 1, 0, 0.5, 1, 0]
    sg[0, 0, 6, :] = [0, 0, 0, 0, 0, 1 / 16.0, 0, 0]
    wm = np.stack([w, mu], -1).astype(t)
    sg = sg.astype(t)
    assert np.array_equal(wm.astype(np.float64), np.stack([w, mu], -1)) or dtype == "f32"
    if dtype == "f32":
        with np.errstate(all="ignore"):
            assert (sg == f32(1e-39)).any() and np.isinf(f32(1) / sg[sg == f32(1e-39)]).all()
    return wm, sg


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_hand_made_volume(pkg, orc, gpu, clean, dtype):
    import torch
    dims = (8, 6, 5)
    wm, sg = hand_made(dtype)
    n = consts(pkg)[1]
    for q in (0.5, 0.25, 1.0, IQR):
        want = stat(pkg, wm, sg, q)
        assert np.isfinite(want).all()
        if q == 0.5:
            # the corner cases are really there, with the answers section 19.1 gives
            assert np.unique(want).size > 100
            row = want[0, 0]
            assert row[0] == 0
            assert f32(0.5) < row[1] <= f32(0.5) + f32(0.5) * f32(2.0 ** -n) + f32(2.0 ** -23)
            assert abs(float(row[2]) - 0.5) <= (0.5 + 10 / 32.0) * 2.0 ** -n + 2.0 ** -23
            assert abs(float(row[3]) - 0.375) <= (10 / 32.0) * 2.0 ** -n + 2.0 ** -23
            assert row[4] == f32(0.625) and row[5] == f32(0.625)
            assert abs(float(row[6]) - 0.5) <= (10 / 16.0) * 2.0 ** -n + 2.0 ** -23
        pkg.init_gmm(wm, sg)
        set_q(pkg, q)
        pkg.bake_gmm_quantile()
        assert_plane(pkg, want, dims, f"hand-made {dtype} q={q}")
        for c in ("C0", "C1"):
            m = cam(pkg, c)
            wf = render_plane(want, W, H, m, density=0.3)
            check(per_step(pkg, torch, m, 0.3), wf, f"hand-made {dtype} {c} q={q} per step")
            check(baked(pkg, torch, m, 0.3), wf, f"hand-made {dtype} {c} q={q} baked")


# ---- the plane ----

@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_plane_values(pkg, orc, gpu, clean, K, dtype):
    """every voxel of the plane, apron duplicates included, is the reference's
    statistic of its record bit for bit; nothing else is written; X = 23 leaves a
    partial last wave in every row at every K; a re-bake gives the same values; the
    single quantile and the spread"""
    (wm, sg), _ = records(orc, DIMS, K, dtype)
    assert pkg.gmm_quantile_info()[1] is None
    pkg.init_gmm(wm, sg)
    sy, sz = plane_pitches(DIMS[0], DIMS[1])
    for q in (QUERIES[K // 16 + 1], IQR):
        set_q(pkg, q)
        assert pkg.gmm_quantile_info()[1] is None   # a new quantile dropped the plane
        pkg.bake_gmm_quantile()
        assert pkg.gmm_quantile_info()[2] == sz * DIMS[2]
        # the other GMM planes are not made
        assert pkg.gmm_stats_info()[1] is None and pkg.gmm_range_info()[1] is None
        want = want_plane(orc, pkg, DIMS, K, dtype, q)
        assert_plane(pkg, want, DIMS, f"K={K} {dtype} q={q}")
        pkg.bake_gmm_quantile()
        assert_plane(pkg, want, DIMS, f"K={K} {dtype} q={q} rebaked")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_baked_frames(pkg, orc, gpu, clean, K, dtype):
    """a frame from the plane equals the reference and the per-step frame of the same
    device at all four cameras; a plane march renders it"""
    import torch
    (wm, sg), _ = records(orc, DIMS, K, dtype)
    pkg.init_gmm(wm, sg)
    for i, c in enumerate(CAMS):
        q = (0.5, IQR)[i % 2]
        density = (0.05, 0.6)[i // 2]
        set_q(pkg, q)
        pkg.bake_gmm_quantile()
        m = cam(pkg, c)
        what = f"K={K} {dtype} {c} q={q} d={density}"
        got = baked(pkg, torch, m, density)
        kernel = pkg.last_kernel()
        assert "<B=1,M=0>" in kernel and kernel.startswith(("k_march_pipe", "k_march_seg")), kernel
        check(got, want_frame(orc, pkg, DIMS, K, dtype, q, c, density), what)
        same(got, per_step(pkg, torch, m, density), what + ": per-step march")
        assert pkg.last_kernel().startswith("k_march_gmm_quant")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_slab_wise_bake(pkg, orc, gpu, clean, dtype):
    """slices [5, 9), [0, 3), [2, 6) uploaded as separate volumes -- out of order,
    overlapping, z_base > 0 -- each baked and freed: the plane and a frame equal
    those of the volume baked at once, rendered with no GMM volume resident"""
    import torch
    K, q = 16, 0.9
    (wm, sg), _ = records(orc, DIMS, K, dtype)
    pkg.set_quantile(q)
    m = cam(pkg, "C1")
    f = Frame(pkg, torch, W, H, m, M11)
    slabs = [(5, 9), (0, 3), (2, 6)]
    seen = set()
    for i, (lo, hi) in enumerate(slabs):
        if i == len(slabs) - 1:
            assert pkg.gmm_quantile_info()[3] == len(seen) == 7
            with pytest.raises(pkg.VRError) as e:
                pkg.render_gmm_baked(f.desc)   # slices missing
            assert e.value.status == pkg._lib.VR_ERR_STATE
        pkg.init_gmm(wm[lo:hi], sg[lo:hi], DIMS, z_base=lo)
        pkg.bake_gmm_quantile()
        pkg.free_gmm()
        seen |= set(range(lo, hi))
        assert pkg.gmm_quantile_info()[3] == len(seen)
    with pytest.raises(pkg.VRError) as e:
        pkg.gmm_info()  # nothing resident
    assert e.value.status == pkg._lib.VR_ERR_STATE
    assert_plane(pkg, want_plane(orc, pkg, DIMS, K, dtype, q), DIMS, "slab-wise")
    pkg.render_gmm_baked(f.desc)
    torch.cuda.synchronize()
    check(f.get(), want_frame(orc, pkg, DIMS, K, dtype, q, "C1", 0.05), "slab-wise frame")


def test_tile_list(pkg, orc, gpu, clean):
    """a shuffled tile list of a 96 x 9 frame cut at 90 columns (2 x 3 tiles, ragged
    right and bottom) with one padding entry and one tile left out: every listed slot
    holds its tile of the whole frame from the plane, which is the per-step frame"""
    import torch
    K, TW, TH = 16, 64, 4
    w, h = 90, 9
    (wm, sg), _ = records(orc, DIMS, K, "f32")
    pkg.init_gmm(wm, sg)
    pkg.set_quantile(0.5)
    pkg.bake_gmm_quantile()
    m = cam(pkg, "C0")
    step = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    pkg.render_gmm(pkg.make_desc(step, w, h, m, query_method=M11, volume_size=(1, 1, 1)))
    pkg.free_gmm()
    whole = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    pkg.render_gmm_baked(pkg.make_desc(whole, w, h, m, query_method=M11, volume_size=(1, 1, 1)))
    torch.cuda.synchronize()
    whole = whole.cpu().numpy().view(np.uint32).reshape(h, w)
    assert whole.any() and not whole.all()  # hits and misses
    assert np.array_equal(whole, step.cpu().numpy().view(np.uint32).reshape(h, w))
    want = render_plane(want_plane(orc, pkg, DIMS, K, "f32", 0.5), w, h, m)["out"]
    assert np.array_equal(whole, want)
    ntiles = 2 * 3
    order = np.random.default_rng(5).permutation(ntiles)[:ntiles - 1].astype(np.uint32)
    tiles = np.insert(order, 3, 0xFFFFFFFF)
    fill = 0x5A5A5A5A
    packed = torch.full((tiles.size * 256,), fill, dtype=torch.int32, device="cuda")
    dl = torch.from_numpy(tiles.view(np.int32).copy()).cuda()
    pkg.render_gmm_baked(pkg.make_desc(packed, w, h, m, query_method=M11, volume_size=(1, 1, 1),
                                       d_tile_list=dl, n_tiles=tiles.size))
    torch.cuda.synchronize()
    assert "<B=1,M=0>" in pkg.last_kernel()
    got = packed.cpu().numpy().view(np.uint32).reshape(tiles.size, TH, TW)
    for slot, t in enumerate(tiles):
        exp = np.full((TH, TW), fill, np.uint32)  # outside the image, padding: untouched
        if t != 0xFFFFFFFF:
            x0, y0 = int(t % 2) * TW, int(t // 2) * TH
            part = whole[y0:y0 + TH, x0:x0 + TW]
            exp[:part.shape[0], :part.shape[1]] = part
        assert np.array_equal(got[slot], exp), f"slot {slot} (tile {t})"


# ---- slab chains ----

@pytest.mark.parametrize("nslabs,c,dtype,q", [(2, "C1", "f32", 0.5), (3, "C0", "f16", IQR)])
def test_slab_chain(pkg, orc, gpu, clean, nslabs, c, dtype, q):
    """each slab resident alone (its slices + halo; the two-slab chain keeps them in
    the two slots), the alive list carried on: the chain ends with no ray alive in
    the whole-volume frame"""
    import torch
    K, density = 16, 0.2
    (wm, sg), _ = records(orc, BIG, K, dtype)
    m = cam(pkg, c)
    bounds = pkg.slabs.slab_bounds(BIG[2], nslabs, pkg.slabs.march_direction(m, W, H))
    set_q(pkg, q)
    f = Frame(pkg, torch, W, H, m, M11, density)
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
        assert pkg.last_kernel().startswith("k_march_gmm_quant") and "M=11" in pkg.last_kernel()
        n_in = int(cnt[0].item())
        carried.append(n_in)
    assert carried[-1] == 0 and carried[0] > 0, carried
    check(f.get(), want_frame(orc, pkg, BIG, K, dtype, q, c, density), f"{nslabs} slabs {c}")


# ---- independence and lifetime ----

def test_three_plane_sets_side_by_side(pkg, orc, gpu, clean):
    """the mean / variance planes, the range plane and the quantile plane resident
    together: releasing any one leaves the other two rendering what they rendered"""
    import torch
    K = 16
    (wm, sg), _ = records(orc, DIMS, K, "f32")
    m = cam(pkg, "C1")
    infos = {"stats": pkg.gmm_stats_info, "range": pkg.gmm_range_info,
             "quantile": pkg.gmm_quantile_info}
    bakes = {"stats": pkg.bake_gmm_stats, "range": pkg.bake_gmm_range,
             "quantile": pkg.bake_gmm_quantile}
    releases = {"stats": pkg.release_gmm_stats, "range": pkg.release_gmm_range,
                "quantile": pkg.release_gmm_quantile}
    methods = {"stats": (1, 2), "range": (10,), "quantile": (M11,)}
    pkg.init_gmm(wm, sg)
    pkg.set_gmm_range(0.25, 0.75)
    pkg.set_quantile(0.5)
    for b in bakes.values():
        b()
    frames = {q: baked(pkg, torch, m, method=q) for qs in methods.values() for q in qs}
    check(frames[M11], want_frame(orc, pkg, DIMS, K, "f32", 0.5, "C1", 0.05), "quantile plane")
    for q in (1, 2, 10):
        same(frames[q], per_step(pkg, torch, m, method=q), f"method {q} beside the quantile plane")
    ptrs = {k: f()[1] for k, f in infos.items()}
    assert all(ptrs.values()) and len(set(ptrs.values())) == 3
    for gone in ("stats", "range", "quantile"):
        releases[gone]()
        assert infos[gone]()[1] is None
        for kept in infos:
            if kept == gone:
                with pytest.raises(pkg.VRError) as e:
                    baked(pkg, torch, m, method=methods[kept][0])
                assert e.value.status == pkg._lib.VR_ERR_STATE
                continue
            assert infos[kept]()[1] == ptrs[kept] and infos[kept]()[3] == DIMS[2]
            for q in methods[kept]:
                same(baked(pkg, torch, m, method=q), frames[q], f"method {q} after releasing {gone}")
        bakes[gone]()
        ptrs[gone] = infos[gone]()[1]
        same(baked(pkg, torch, m, method=methods[gone][0]), frames[methods[gone][0]],
             f"{gone} baked again")
    # a change of the range drops the range plane only
    pkg.set_gmm_range(0.4, 0.5)
    assert pkg.gmm_range_info()[1] is None and pkg.gmm_quantile_info()[1] == ptrs["quantile"]
    same(baked(pkg, torch, m), frames[M11], "after a new range")


def test_quantile_setters_drop_only_the_quantile_planes(pkg, orc, gpu, clean):
    """set_quantile, set_quantile_spread and the clear drop the GMM quantile plane (and
    the histogram-side one, as before), not the other GMM planes; the plane survives
    free_gmm, gmm_select and another volume"""
    import torch
    K = 16
    (wm, sg), _ = records(orc, DIMS, K, "f16")
    m = cam(pkg, "C0")
    pkg.init_gmm(wm, sg)
    pkg.set_gmm_range(0.25, 0.75)
    pkg.bake_gmm_stats()
    pkg.bake_gmm_range()
    others = (pkg.gmm_stats_info(), pkg.gmm_range_info())
    hist = orc.synth_volume(12, 10, 8, 8)
    pkg.init_distribution(hist)
    for change in (lambda: pkg.set_quantile(0.5), lambda: pkg.set_quantile_spread(*IQR),
                   lambda: pkg.set_quantile(None), lambda: pkg.set_quantile(0.5)):
        pkg.set_quantile(0.9)
        pkg.bake_gmm_quantile()
        pkg.bake_quantile()
        assert pkg.gmm_quantile_info()[1] and pkg.quantile_info()[0]
        change()
        assert pkg.gmm_quantile_info() == ((0, 0, 0), None, 0, 0)
        assert pkg.quantile_info()[0] is None
        assert (pkg.gmm_stats_info(), pkg.gmm_range_info()) == others
    pkg.release_stats()
    # survives the records' departure, a change of slot and another volume
    pkg.bake_gmm_quantile()
    info = pkg.gmm_quantile_info()
    want = want_frame(orc, pkg, DIMS, K, "f16", 0.5, "C0", 0.05)
    pkg.free_gmm()
    check(baked(pkg, torch, m), want, "no records resident")
    pkg.gmm_select(1)
    pkg.synthesize_gmm((16, 16, 16), 8)
    assert pkg.gmm_quantile_info() == info
    check(baked(pkg, torch, m), want, "another volume in slot 1")
    pkg.convert_gmm_f16()
    pkg.gmm_select(0)
    assert pkg.gmm_quantile_info() == info
    check(baked(pkg, torch, m), want, "back on slot 0")
    pkg.freeCudaBuffers()
    assert pkg.gmm_quantile_info()[1] is None
    assert pkg.gmm_stats_info()[1] is None and pkg.gmm_range_info()[1] is None
    assert pkg.quantile() == (0.5, 0.5, False)   # the quantile is host state: it stays


# ---- states ----

def test_states_and_errors(pkg, orc, gpu, clean):
    import torch
    E = pkg._lib
    K = 16
    (wm, sg), _ = records(orc, DIMS, K, "f32")
    m = cam(pkg, "C1")
    f = Frame(pkg, torch, W, H, m, M11)
    pkg.init_gmm(wm, sg)
    before = [per_step(pkg, torch, m, method=q) for q in (1, 2)]
    for call in (pkg.render_gmm, pkg.render_gmm_baked, lambda d: pkg.bake_gmm_quantile()):
        with pytest.raises(pkg.VRError) as e:
            call(f.desc)  # no quantile (and no plane)
        assert e.value.status == E.VR_ERR_STATE
    pkg.set_quantile(0.5)
    with pytest.raises(pkg.VRError) as e:
        pkg.render_gmm_baked(f.desc)  # a quantile, no plane
    assert e.value.status == E.VR_ERR_STATE
    with pytest.raises(pkg.VRError) as e:
        pkg.gmm_count_footprint(f.desc)  # no counting instance of the quantile
    assert e.value.status == E.VR_ERR_UNSUPPORTED
    for method in (3, 7):
        for call in (pkg.render_gmm, pkg.render_gmm_baked):
            with pytest.raises(pkg.VRError) as e:
                call(Frame(pkg, torch, W, H, m, method).desc)
            assert e.value.status == E.VR_ERR_UNSUPPORTED
    # methods 1 / 2 render what they rendered, with a quantile set and its plane resident
    pkg.bake_gmm_quantile()
    for q in (1, 2):
        same(per_step(pkg, torch, m, method=q), before[q - 1], f"method {q} with a quantile set")
        assert pkg.last_kernel().startswith("k_march_gmm<")
    assert pkg.gmm_count_footprint(Frame(pkg, torch, W, H, m, 1).desc) > 0
    want = want_frame(orc, pkg, DIMS, K, "f32", 0.5, "C1", 0.05)
    check(baked(pkg, torch, m), want, "baked quantile frame")
    # refused bakes leave the plane as it is
    pkg.gmm_select(1)
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_gmm_quantile()  # slot 1 is empty
    assert e.value.status == E.VR_ERR_STATE
    pkg.synthesize_gmm((16, 16, 16), 8)
    with pytest.raises(pkg.VRError) as e:
        pkg.bake_gmm_quantile()  # other dims onto the existing plane
    assert e.value.status == E.VR_ERR_STATE
    pkg.free_gmm()
    pkg.gmm_select(0)
    assert_plane(pkg, want_plane(orc, pkg, DIMS, K, "f32", 0.5), DIMS, "after the refused bakes")
    check(baked(pkg, torch, m), want, "after the refused bakes")
    # the release keeps the quantile; other dims bake after it
    pkg.release_gmm_quantile()
    assert pkg.gmm_quantile_info()[1] is None and pkg.quantile() == (0.5, 0.5, False)
    with pytest.raises(pkg.VRError) as e:
        pkg.render_gmm_baked(f.desc)
    assert e.value.status == E.VR_ERR_STATE
    pkg.synthesize_gmm((16, 16, 16), 8)
    pkg.bake_gmm_quantile()
    assert pkg.gmm_quantile_info()[0] == (16, 16, 16)
