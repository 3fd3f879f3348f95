"""GPU checks of the 2-D transfer function over two planes (vr_transfer2.hip,
DESIGN.md section 23).

The classifier is float arithmetic in a fixed order which numpy float32 restates
bit for bit (tests/ref_transfer2.py), so every comparison is exact: packed RGBA8,
float RGBA and samples per pixel are np.array_equal, no tolerance and no pixel left
out.  Two references: the library's own frames under the built-in table (a table
whose rows are the reference's nine entries must reproduce them through the new
kernel, whatever plane v is), and test_transfer2.py's numpy frames, which that
file checks on the CPU.  The GMM frames are marched by numpy over the planes the
device holds (their values are tests/test_gpu_gmm_*.py's business).
"""
import numpy as np
import pytest

import ref_transfer2
from test_crossing import BAKE, DIMS, H, THETA, W, camera, volume
from test_gpu_crossing import (GH, GW, PAD, SENTINEL, assert_same, gmm_records, render)
from test_gpu_f16 import d2h
from test_gpu_gmm_baked import unbrick
from test_transfer import RAMP2, RAND256
from test_transfer import reference as reference_1d
from test_transfer2 import (CODEC, FRAMES, PAIRS, RAMP22, RAND32, T255X4, TABLES, blend_of,
                            codec_records, plane, reference)

pytestmark = pytest.mark.gpu


def kernel_of(u, v):
    return f"k_march_tf2<B=2,M={int(u == 13) + 2 * int(v == 13)}>"


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    def clear():
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


def upload_planes(pkg, dims, nb, dtype):
    """the records resident with the planes of methods 1/2/3, 10 (F: the weights of
    [0, THETA)), 11 (the median) and 13 (F) baked"""
    pkg.init_distribution(volume(dims, nb, dtype))
    pkg.set_query_range(0.0, THETA, nb)
    pkg.set_quantile(0.5)
    pkg.set_isovalue(THETA, nb)
    pkg.bake_stats()
    pkg.bake_weighted()
    pkg.bake_quantile()
    pkg.bake_crossing()


def set_pair(pkg, pair, table):
    """the 2-D table of the pair; returns (u, the kernel's name)"""
    u, v, voff, vscale = PAIRS[pair]
    pkg.set_transfer_function_2d(TABLES[table], v, voff, vscale)
    return u, kernel_of(u, v)


def ref(pair, table, dims, nb, dtype, cam, w, h):
    return reference(pair, table, dims, nb, dtype, cam, w, h)[:3]


# ---- 1. identity: rows of the reference's nine entries through the new kernel ----

def identity(pkg, frame, v, new_kernel, what):
    pkg.set_transfer_function_2d(None)
    want = frame()
    old = pkg.last_kernel()
    assert "k_march_tf2" not in old, old
    pkg.set_transfer_function_2d(np.repeat(pkg.REFERENCE_TF[None], 3, axis=0), v, 0.1, 1.3)
    copies = pkg.layout_info()["resident_bytes"]
    got = frame()
    assert pkg.last_kernel() == new_kernel, (what, pkg.last_kernel())
    assert pkg.layout_info()["resident_bytes"] == copies  # no layout copy made
    hit = want[2] >= 0
    assert hit.sum() > 100 and np.unique(want[0][hit]).size > 1, what
    assert_same(got, want, what)


def test_identity_record_planes(pkg, gpu):
    """u in 1/2/3 and 10/11/12/13, v another plane each time"""
    import torch
    vol = volume(DIMS, 8, "f32")
    upload_planes(pkg, DIMS, 8, "f32")
    pkg.set_query_target(np.asarray(vol[8, 10, 12]), "emd")
    pkg.bake_distance()
    methods = (1, 2, 3, 10, 11, 12, 13)
    for c, cam in enumerate(("C0", "C1")):
        for k, u in enumerate(methods):
            v = methods[(k + 1 + 2 * c) % len(methods)]
            identity(pkg, lambda: render(pkg, torch, W, H, camera(cam), method=u), v,
                     kernel_of(u, v), f"u {u} v {v} {cam}")


def test_identity_codec_planes(pkg, gpu):
    """u in 4/5/6 of a codec volume's planes, v another of them"""
    import torch
    pkg.init_codec(*codec_records())
    pkg.bake_stats()
    for c, cam in enumerate(("C0", "C1")):
        for u in (4, 5, 6):
            v = 4 + (u - 4 + 1 + c) % 3
            identity(pkg, lambda: render(pkg, torch, W, H, camera(cam), method=u), v,
                     kernel_of(u, v), f"codec u {u} v {v} {cam}")


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
    """render_gmm_baked u in 1, 2, 10, 11 and 13 of the K = 16 volume, v another"""
    import torch
    bake_gmm_planes(pkg)
    try:
        pkg.free_gmm()  # the planes need no records
        methods = (1, 2, 10, 11, 13)
        for c, cam in enumerate(("C0", "C1")):
            for k, u in enumerate(methods):
                v = methods[(k + 1 + c) % len(methods)]
                identity(pkg, lambda: gmm_frame(pkg, torch, camera(cam), u), v, kernel_of(u, v),
                         f"GMM u {u} v {v} {cam}")
    finally:
        pkg.set_transfer_function_2d(None)
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
    """every pair of the record volumes and every table (test_transfer2.FRAMES)"""
    import torch
    dims, nb, dtype, cam, w, h = case
    upload_planes(pkg, dims, nb, dtype)
    for pair, table in FRAMES:
        u, kernel = set_pair(pkg, pair, table)
        got = render(pkg, torch, w, h, camera(cam), method=u)
        assert pkg.last_kernel() == kernel
        assert_same(got, ref(pair, table, dims, nb, dtype, cam, w, h), f"{pair} {table} {case}")
    assert pkg.layout_info()["resident_bytes"] == 0  # no layout copy is used or made


@pytest.mark.parametrize("cam", ("C0", "C1", "S"))
def test_codec_pair_against_numpy(pkg, gpu, cam):
    """u = 4 (mean), v = 6 (entropy) of the codec volume's planes"""
    import torch
    pkg.init_codec(*codec_records())
    pkg.bake_stats()
    for table in ("rand32", "ramp22"):
        u, kernel = set_pair(pkg, "4-6", table)
        got = render(pkg, torch, W, H, camera(cam), method=u)
        assert pkg.last_kernel() == kernel
        assert_same(got, ref("4-6", table, CODEC, 8, "f32", cam, W, H), f"codec {table} {cam}")


def test_offsets_and_scales(pkg, gpu):
    """xu = (su - transfer_offset) * transfer_scale, xv = (sv - v_offset) * v_scale,
    with another density and brightness"""
    import torch
    upload_planes(pkg, DIMS, 8, "f32")
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    for (u, v), table, toff, tscale, voff, vscale in (((1, 13), RAND32, 0.05, 2.5, 0.2, 1.7),
                                                      ((13, 2), T255X4, 0.1, 1.7, 0.3, -4.0)):
        pkg.set_transfer_function_2d(table, v, voff, vscale)
        pkg.render(pkg.make_desc(out, W, H, camera("C1"), query_method=u, density=0.2,
                                 brightness=1.5, transfer_offset=toff, transfer_scale=tscale))
        torch.cuda.synchronize()
        assert pkg.last_kernel() == kernel_of(u, v)
        want = ref_transfer2.render_planes(
            plane(DIMS, 8, "f32", u), plane(DIMS, 8, "f32", v), W, H, camera("C1"), table,
            blend_u=blend_of(u), blend_v=blend_of(v), voff=voff, vscale=vscale, density=0.2,
            brightness=1.5, toff=toff, tscale=tscale)[0]
        assert np.unique(want).size > 100
        assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(H, W), want), (u, v)


# ---- 3. both addressing modes ----

def test_wide_addressing_changes_no_pixel(pkg, gpu, tune):
    import torch
    for dims, nb, dtype in ((DIMS, 8, "f32"), (BAKE, 4, "f16")):
        upload_planes(pkg, dims, nb, dtype)
        for pair, table in (("1-13", "rand32"), ("13-2", "t255x4")):
            u, kernel = set_pair(pkg, pair, table)
            tune.clear("VR_TF_WIDE")
            narrow = render(pkg, torch, W, H, camera("C1"), method=u)
            tune.set("VR_TF_WIDE", "1")
            wide = render(pkg, torch, W, H, camera("C1"), method=u)
            assert pkg.last_kernel() == kernel
            assert_same(wide, narrow, f"VR_TF_WIDE {dims} {pair}")
            assert_same(wide, ref(pair, table, dims, nb, dtype, "C1", W, H), "wide")
        tune.clear("VR_TF_WIDE")


# ---- 4. inherited launch features ----

LAUNCH_PAIRS = (("1-13", "rand32"), ("13-2", "t255x4"))


@pytest.mark.parametrize("pair,table", LAUNCH_PAIRS)
def test_tile_list_with_padding_and_a_miss_tile(pkg, gpu, pair, table):
    """test_gpu_crossing.py's list of the 70 x 50 frame: tiles that hit, a padding
    entry (its slot stays untouched: the workgroup leaves after the staging barrier),
    a tile of misses only and right-edge tiles"""
    import torch
    fw, fh = 70, 50
    upload_planes(pkg, DIMS, 8, "f32")
    u, kernel = set_pair(pkg, pair, table)
    ref8, reff, refn = ref(pair, table, DIMS, 8, "f32", "C1", fw, fh)
    tiles = [12, PAD, 24, 13, 15, 1]
    assert np.all(refn[48:50, 0:64] < 0), "tile 24 must be a miss tile"
    n = len(tiles)
    dl = torch.from_numpy(np.array(tiles, np.uint32).view(np.int32)).cuda()
    out = torch.full((n * 256,), SENTINEL, dtype=torch.int32, device="cuda")
    out_f = torch.full((n * 256 * 4,), -7.0, dtype=torch.float32, device="cuda")
    steps = torch.full((n * 256,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, fw, fh, camera("C1"), query_method=u, d_output_f=out_f,
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


@pytest.mark.parametrize("pair,table", LAUNCH_PAIRS)
def test_render_kernel_partial_coverage(pkg, gpu, pair, table):
    """a grid of 3 x 5 blocks of 16 x 4 threads covers 48 x 20 pixels of the 64 x 48
    image: those equal the reference, every other pixel keeps its sentinel"""
    import torch
    upload_planes(pkg, DIMS, 8, "f32")
    u, kernel = set_pair(pkg, pair, table)
    pkg.copyInvViewMatrix(camera("C0"))
    out = torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda")
    pkg.render_kernel((3, 5, 1), (16, 4, 1), out, W, H, 0.05, 1.0, 0.0, 1.0, u, DIMS)
    torch.cuda.synchronize()
    assert pkg.last_kernel() == kernel
    got = out.cpu().numpy().view(np.uint32).reshape(H, W)
    ref8, _, refn = ref(pair, table, DIMS, 8, "f32", "C0", W, H)
    want = np.full((H, W), SENTINEL, np.uint32)
    want[:20, :48] = np.where(refn[:20, :48] >= 0, ref8[:20, :48], SENTINEL)
    assert (refn[:20, :48] >= 0).any() and (refn[:20, :48] < 0).any()
    assert np.array_equal(got, want), int(np.sum(got != want))


@pytest.mark.parametrize("cap", ("1", "3", "7"))
def test_wg_per_cu_changes_no_pixel(pkg, gpu, tune, cap):
    """the cap's LDS request, less the table's static 16 KiB: a scheduling knob only"""
    import torch
    tune.set("VR_WG_PER_CU", cap)
    upload_planes(pkg, DIMS, 8, "f32")
    for pair, table in LAUNCH_PAIRS:
        u, kernel = set_pair(pkg, pair, table)
        got = render(pkg, torch, W, H, camera("C0"), method=u)
        assert pkg.last_kernel() == kernel
        assert_same(got, ref(pair, table, DIMS, 8, "f32", "C0", W, H), f"cap {cap} {pair}")


# ---- 5. table changes ----

@pytest.mark.parametrize("own_stream", (False, True))
def test_table_changes_reach_the_device(pkg, gpu, own_stream):
    """A, B, A again, then a 1-D table, then the 2-D table again: a stale device copy
    of either kind would repeat a frame"""
    import torch
    upload_planes(pkg, DIMS, 8, "f32")
    stream = torch.cuda.Stream() if own_stream else None
    try:
        pkg.set_stream(stream)
        frames = []
        for table in ("ramp22", "rand32", "ramp22", "1d", "rand32", "1d", "ramp22"):
            if table == "1d":
                pkg.set_transfer_function(RAND256)
                assert pkg.transfer_function_2d() is None
                u = 13
            else:
                u, _ = set_pair(pkg, "1-13", table)
                assert pkg.transfer_function() is None
            with torch.cuda.stream(stream) if own_stream else torch.cuda.stream(None):
                frames.append((table, render(pkg, torch, W, H, camera("C1"), method=u),
                               pkg.last_kernel()))
        for table, got, kernel in frames:
            if table == "1d":
                assert kernel == "k_march_plane_tf<B=1,M=13>"
                want = reference_1d(DIMS, 8, "f32", "C1", W, H, "rand256", "combine")[:3]
            else:
                assert kernel == kernel_of(1, 13)
                want = ref("1-13", table, DIMS, 8, "f32", "C1", W, H)
            assert_same(got, want, table)
        assert_same(frames[2][1], frames[0][1], "A again")
        assert not np.array_equal(frames[1][1][0], frames[0][1][0])
        # back on the default stream after frames on another one
        pkg.set_stream(None)
        u, _ = set_pair(pkg, "13-2", "t255x4")
        got = render(pkg, torch, W, H, camera("C1"), method=u)
        assert_same(got, ref("13-2", "t255x4", DIMS, 8, "f32", "C1", W, H), "default stream")
    finally:
        torch.cuda.synchronize()
        pkg.set_stream(None)


# ---- 6. lifetime ----

def _table_state(pkg):
    t = pkg.transfer_function_2d()
    return None if t is None else (t[0].tobytes(),) + t[1:]


def test_lifetime(pkg, gpu):
    import torch
    upload_planes(pkg, DIMS, 8, "f32")
    planes = (pkg.weighted_info(), pkg.crossing_info(), pkg.quantile_info(), pkg.stats_info())
    assert planes[0][0] and planes[1][0]
    before = pkg.layout_info()["resident_bytes"]
    u, _ = set_pair(pkg, "1-13", "rand32")
    keep = _table_state(pkg)

    def resident():
        return (pkg.weighted_info(), pkg.crossing_info(), pkg.quantile_info(), pkg.stats_info())

    assert resident() == planes  # setting drops no plane
    want = ref("1-13", "rand32", DIMS, 8, "f32", "C1", W, H)
    assert_same(render(pkg, torch, W, H, camera("C1"), method=u), want, "first")
    set_pair(pkg, "13-2", "t255x4")
    set_pair(pkg, "1-13", "rand32")
    assert resident() == planes
    assert pkg.layout_info()["resident_bytes"] == before
    # freeCudaBuffers frees the device copy and every plane; the table stays set and
    # is uploaded again for the next frame, of a new upload
    pkg.freeCudaBuffers()
    assert _table_state(pkg) == keep
    assert pkg.crossing_info() == (None, 0)
    upload_planes(pkg, DIMS, 8, "f32")
    assert_same(render(pkg, torch, W, H, camera("C1"), method=u), want, "after freeCudaBuffers")
    # a new volume, vr_convert_f16 and the releases keep it too
    pkg.convert_f16()
    pkg.release_crossing()
    pkg.release_stats()
    assert _table_state(pkg) == keep
    pkg.bake_stats()
    pkg.bake_crossing()
    assert_same(render(pkg, torch, W, H, camera("C1"), method=u),
                ref("1-13", "rand32", DIMS, 8, "f16", "C1", W, H), "after vr_convert_f16")
    assert pkg.layout_info()["resident_bytes"] == before


# ---- 7. GMM volumes ----

def _gmm_plane(info, k=0):
    """plane k of a baked GMM set as the device holds it, (Z, Y, X) float32"""
    dims, ptr, n, nbaked = info
    assert ptr and nbaked == dims[2]
    raw = d2h(ptr + 4 * n * k, n, np.float32)
    return unbrick(raw[None], dims)[0][0]


def test_gmm_pairs(pkg, gpu):
    """(1, 13): the mean coloured, fading by the crossing combine of the range plane;
    (11, 2): the median against 16 x variance -- from the K = 16 volume's planes with
    the records freed"""
    import torch
    lib = pkg._lib
    bake_gmm_planes(pkg)
    try:
        pkg.free_gmm()
        planes = {1: _gmm_plane(pkg.gmm_stats_info(), 0), 2: _gmm_plane(pkg.gmm_stats_info(), 1),
                  13: _gmm_plane(pkg.gmm_range_info()), 11: _gmm_plane(pkg.gmm_quantile_info())}
        # (the oracle's 16 x variance of these records lies in [0.03, 0.13]: the window)
        for (u, v), table, voff, vscale in (((1, 13), RAND32, 0.0, 1.0),
                                            ((11, 2), T255X4, 0.03, 10.0)):
            pkg.set_transfer_function_2d(table, v, voff, vscale)
            for cam in ("C0", "C1"):
                want = ref_transfer2.render_planes(planes[u], planes[v], GW, GH, camera(cam), table,
                                                   blend_u=blend_of(u), blend_v=blend_of(v),
                                                   voff=voff, vscale=vscale)
                flat = ref_transfer2.render_planes(planes[u], planes[v], GW, GH, camera(cam),
                                                   np.repeat(table[:1], table.shape[0], axis=0),
                                                   blend_u=blend_of(u), blend_v=blend_of(v),
                                                   voff=voff, vscale=vscale)
                hit = want[2] >= 0
                differ = int((want[0] != flat[0])[hit].sum())
                print(f"GMM {u}-{v} {cam}: {int(hit.sum())} hit, {differ} differ from row 0")
                assert hit.sum() > 1000 and 4 * differ >= hit.sum()
                got = gmm_frame(pkg, torch, camera(cam), u)
                assert pkg.last_kernel() == kernel_of(u, v)
                assert_same(got, want, f"GMM {u}-{v} {cam}")
        # a v plane set that is not resident: the table's refusal; a codec v: no GMM plane
        pkg.release_gmm_quantile()
        for v in (11, 4, 12):
            pkg.set_transfer_function_2d(RAMP22, v)
            with pytest.raises(pkg.VRError) as e:
                gmm_frame(pkg, torch, camera("C0"), 1)
            assert e.value.status == lib.VR_ERR_UNSUPPORTED, v
            assert "custom transfer function" in str(e.value) and "bake" in str(e.value)
        pkg.set_transfer_function_2d(RAMP22, 2)
        with pytest.raises(pkg.VRError) as e:  # and u's
            gmm_frame(pkg, torch, camera("C0"), 11)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
    finally:
        pkg.set_transfer_function_2d(None)
        pkg.release_gmm_stats()
        pkg.release_gmm_range()
        pkg.release_gmm_quantile()


# ---- 8. refusals ----

def test_refusals(pkg, gpu):
    """with a 2-D table set nothing falls back to the built-in table or to the 1-D
    route: a v plane that is not baked, a pair of two families and what has no plane
    march are VR_ERR_UNSUPPORTED, and all succeed as before once the table is cleared"""
    import torch
    lib = pkg._lib
    pkg.init_distribution(volume(DIMS, 8, "f32"))
    pkg.set_query_range(0.0, THETA, 8)
    pkg.set_isovalue(THETA, 8)
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
        "method 13 per step": lambda: render(pkg, torch, W, H, m, method=13),
        "method 7": lambda: render(pkg, torch, W, H, m, method=7),
        "render_gmm": gmm_render,
        "count_footprint": lambda: pkg.count_footprint(d1),
    }

    def refused(f, what):
        with pytest.raises(pkg.VRError) as e:
            f()
        assert e.value.status == lib.VR_ERR_UNSUPPORTED, what
        assert "custom transfer function" in str(e.value) and "bake" in str(e.value), what

    try:
        before = {k: f() for k, f in calls.items()}
        pkg.set_transfer_function_2d(RAMP22, 13)
        for k, f in calls.items():
            refused(f, k)
        # u baked, v not
        pkg.bake_stats()
        refused(lambda: render(pkg, torch, W, H, m, method=1), "v = 13 not baked")
        refused(lambda: render(pkg, torch, W, H, m, method=7), "method 7 from the planes")
        pkg.bake_crossing()
        got = render(pkg, torch, W, H, m, method=1)  # both resident: a frame
        assert pkg.last_kernel() == kernel_of(1, 13) and (got[2] >= 0).any()
        refused(lambda: render(pkg, torch, W, H, m, method=10), "u = 10 not baked")
        # a mixed family: u of the record planes, v of the codec planes
        pkg.set_transfer_function_2d(RAMP22, 4)
        refused(lambda: render(pkg, torch, W, H, m, method=1), "pair (1, 4)")
        # a 1-D table set over it is the 1-D route again, and the other way round
        pkg.set_transfer_function(RAMP2)
        render(pkg, torch, W, H, m, method=13)
        assert pkg.last_kernel() == "k_march_plane_tf<B=1,M=13>"
        pkg.set_transfer_function_2d(RAMP22, 13)
        render(pkg, torch, W, H, m, method=13)
        assert pkg.last_kernel() == kernel_of(13, 13)
        pkg.release_stats()
        pkg.set_query_range(0.0, THETA, 8)
        pkg.set_isovalue(THETA, 8)
        pkg.set_transfer_function_2d(None)
        for k, f in calls.items():
            after = f()
            if isinstance(after, tuple):
                assert_same(after, before[k], k)
            else:
                assert np.array_equal(after, before[k]), k
    finally:
        pkg.set_transfer_function_2d(None)
        pkg.free_gmm()
