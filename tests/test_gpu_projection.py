"""GPU checks of the ray projections (vr_project.hip).

The march, the three reductions and the one classification per ray are float
arithmetic in a fixed order which numpy float32 restates bit for bit
(tests/ref_projection.py), so every comparison is exact: packed RGBA8, float RGBA and
samples per pixel are np.array_equal, no tolerance and no pixel left out.  The
reference frames are test_projection.py's, which that file checks on the CPU.  The
shapes are small on purpose: BAKE's 5 x 3 rows clamp footprints, the views have
one-sample rays and rays of 296 samples that wrap the ring of sets in flight many
times and end in every position of it, and waves at the silhouette mix both, so
both the whole rounds and the predicated rest of the kernel run.
"""
import numpy as np
import pytest

from test_crossing import BAKE, DIMS, H, THETA, W, camera, cdf, volume
from test_gpu_crossing import GH, GW, PAD, SENTINEL, assert_same, gmm_records, render
from test_gpu_transfer import bake_gmm_planes, gmm_frame, upload_F_planes
from test_projection import MODES, reference
from test_transfer import N255, RAMP2, RAND256, TABLES

pytestmark = pytest.mark.gpu

# the two planes of F the numpy frames are marched over: method 10's (blended) and
# method 13's (combined)
PLANES = ((10, "trilinear", False), (13, "combine", True))


def kernel(mode, cross):
    return f"k_march_proj_{mode}<B=1,M={13 if cross else 0}>"


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    def clear():
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
    + [(BAKE, 4, "f32", cam, W, H) for cam in ("C0", "C1", "S")] + [(BAKE, 4, "f16", "C1", W, H)]
)


@pytest.mark.parametrize("case", NUMPY_CASES, ids=lambda c: "-".join(
    "x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c))
def test_against_numpy(pkg, gpu, case):
    """all three modes under ramp2, rand256, the one-entry and the 255-entry table and
    no table, on the method-10 and the method-13 plane"""
    import torch
    dims, nb, dtype, cam, w, h = case
    upload_F_planes(pkg, dims, nb, dtype)
    for name in ("ramp2", "rand256", "one", "n255", None):
        set_table(pkg, name)
        for mode in MODES:
            pkg.set_projection(mode)
            for method, blend, cross in PLANES:
                got = render(pkg, torch, w, h, camera(cam), method=method)
                assert pkg.last_kernel() == kernel(mode, cross)
                assert_same(got, reference(dims, nb, dtype, cam, w, h, name, blend, mode),
                            f"{mode} {name} method {method} {case}")
    assert pkg.layout_info()["resident_bytes"] == 0  # no layout copy is used or made


# ---- 2. no table is the reference's nine entries ----

def identity(pkg, frame, cross, what):
    for mode in MODES:
        pkg.set_projection(mode)
        pkg.set_transfer_function(None)
        copies = pkg.layout_info()["resident_bytes"]
        want = frame()
        assert pkg.last_kernel() == kernel(mode, cross), (what, pkg.last_kernel())
        pkg.set_transfer_function(pkg.REFERENCE_TF)
        got = frame()
        assert pkg.last_kernel() == kernel(mode, cross), (what, pkg.last_kernel())
        assert pkg.layout_info()["resident_bytes"] == copies  # no layout copy made
        assert (want[2] >= 0).sum() > 100, what
        assert_same(got, want, f"{what} {mode}")
    pkg.set_transfer_function(None)


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
    colours = 0
    for method in (1, 2, 3, 10, 11, 12, 13):
        identity(pkg, lambda: render(pkg, torch, W, H, camera("C1"), method=method), method == 13,
                 f"method {method}")
        pkg.set_projection("mean")
        f = render(pkg, torch, W, H, camera("C1"), method=method)
        colours = max(colours, np.unique(f[0][f[2] >= 0]).size)
    assert colours > 10


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
        pkg.set_projection(None)
        pkg.set_transfer_function(None)
        pkg.release_gmm_stats()


# ---- 3. the samples are those of the existing march under a transparent table ----

def test_samples_per_pixel_are_k_march_plane_tf_s(pkg, gpu):
    import torch
    clear = RAND256.copy()
    clear[:, 3] = 0
    for dims, nb in ((DIMS, 8), (BAKE, 4)):
        upload_F_planes(pkg, dims, nb, "f32")
        for cam in ("C0", "C1", "S"):
            for method, _, cross in PLANES:
                pkg.set_projection(None)
                pkg.set_transfer_function(clear)
                want = render(pkg, torch, W, H, camera(cam), method=method)
                assert pkg.last_kernel().startswith("k_march_plane_tf<"), pkg.last_kernel()
                assert (want[2] >= 0).sum() > 50 and not want[0].any()
                for mode in MODES:
                    pkg.set_projection(mode)
                    got = render(pkg, torch, W, H, camera(cam), method=method)
                    assert pkg.last_kernel() == kernel(mode, cross)
                    assert np.array_equal(got[2], want[2]), (dims, cam, method, mode)


# ---- 4. the descriptor's parameters ----

def test_window_and_brightness_are_honoured_and_density_is_not_read(pkg, gpu):
    import torch
    import ref_crossing
    import ref_projection
    upload_F_planes(pkg, DIMS, 8, "f32")
    pkg.set_transfer_function(RAND256)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    for mode in MODES:
        pkg.set_projection(mode)
        for method, blend in ((10, ref_crossing.trilinear), (13, ref_crossing.combine)):
            frames = []
            for density in (0.05, 0.9):
                pkg.render(pkg.make_desc(out, W, H, camera("C1"), query_method=method,
                                         density=density, brightness=1.5, transfer_offset=0.1,
                                         transfer_scale=1.7))
                torch.cuda.synchronize()
                frames.append(out.cpu().numpy().view(np.uint32).reshape(H, W).copy())
            want = ref_projection.render_plane(cdf(DIMS, 8, "f32"), W, H, camera("C1"), mode,
                                               RAND256, blend=blend, brightness=1.5, toff=0.1,
                                               tscale=1.7)[0]
            assert np.array_equal(frames[0], want), (mode, method)
            assert np.array_equal(frames[1], want), (mode, method, "density")
            plain = reference(DIMS, 8, "f32", "C1", W, H, "rand256",
                              "trilinear" if method == 10 else "combine", mode)[0]
            assert (want != plain).sum() > 500


# ---- 5. both addressing modes, occupancy caps ----

def test_wide_addressing_changes_no_pixel(pkg, gpu, tune):
    import torch
    for dims, nb, dtype in ((DIMS, 8, "f32"), (BAKE, 4, "f16")):
        upload_F_planes(pkg, dims, nb, dtype)
        pkg.set_transfer_function(RAND256)
        for mode in MODES:
            pkg.set_projection(mode)
            for method, blend, cross in PLANES:
                tune.clear("VR_TF_WIDE")
                narrow = render(pkg, torch, W, H, camera("C1"), method=method)
                tune.set("VR_TF_WIDE", "1")
                wide = render(pkg, torch, W, H, camera("C1"), method=method)
                assert pkg.last_kernel() == kernel(mode, cross)
                assert_same(wide, narrow, f"VR_TF_WIDE {dims} {mode} method {method}")
                assert_same(wide, reference(dims, nb, dtype, "C1", W, H, "rand256", blend, mode),
                            "wide")
        tune.clear("VR_TF_WIDE")


@pytest.mark.parametrize("cap", ("1", "3", "7"))
def test_wg_per_cu_changes_no_pixel(pkg, gpu, tune, cap):
    import torch
    tune.set("VR_WG_PER_CU", cap)
    upload_F_planes(pkg, DIMS, 8, "f32")
    pkg.set_transfer_function(RAND256)
    for mode in MODES:
        pkg.set_projection(mode)
        for method, blend, cross in PLANES:
            got = render(pkg, torch, W, H, camera("C0"), method=method)
            assert pkg.last_kernel() == kernel(mode, cross)
            assert_same(got, reference(DIMS, 8, "f32", "C0", W, H, "rand256", blend, mode),
                        f"cap {cap} {mode}")


# ---- 6. inherited launch features ----

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("method,blend,cross", PLANES)
def test_tile_list_with_padding_and_a_miss_tile(pkg, gpu, method, blend, cross, mode):
    """test_gpu_crossing.py's list of the 70 x 50 frame: tiles that hit, a padding
    entry (its slot stays untouched), a tile of misses only and right-edge tiles"""
    import torch
    fw, fh = 70, 50
    upload_F_planes(pkg, DIMS, 8, "f32")
    pkg.set_transfer_function(RAND256)
    pkg.set_projection(mode)
    ref8, reff, refn = reference(DIMS, 8, "f32", "C1", fw, fh, "rand256", blend, mode)
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
    assert pkg.last_kernel() == kernel(mode, cross)
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
    upload_F_planes(pkg, DIMS, 8, "f32")
    pkg.set_transfer_function(RAMP2)
    pkg.copyInvViewMatrix(camera("C0"))
    for mode in MODES:
        pkg.set_projection(mode)
        out = torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda")
        pkg.render_kernel((3, 5, 1), (16, 4, 1), out, W, H, 0.05, 1.0, 0.0, 1.0, method, DIMS)
        torch.cuda.synchronize()
        assert pkg.last_kernel() == kernel(mode, cross)
        got = out.cpu().numpy().view(np.uint32).reshape(H, W)
        ref8, _, refn = reference(DIMS, 8, "f32", "C0", W, H, "ramp2", blend, mode)
        want = np.full((H, W), SENTINEL, np.uint32)
        want[:20, :48] = np.where(refn[:20, :48] >= 0, ref8[:20, :48], SENTINEL)
        assert (refn[:20, :48] >= 0).any() and (refn[:20, :48] < 0).any()
        assert np.array_equal(got, want), (mode, int(np.sum(got != want)))


# ---- 7. mode and table changes ----

@pytest.mark.parametrize("own_stream", (False, True))
def test_mode_changes_reach_the_next_frame(pkg, gpu, own_stream):
    """max, mean, max again, with table changes in between (the built-in table's device
    copy and the caller's are two buffers)"""
    import torch
    upload_F_planes(pkg, DIMS, 8, "f32")
    stream = torch.cuda.Stream() if own_stream else None
    try:
        pkg.set_stream(stream)
        frames = []
        for mode, name in (("max", "rand256"), ("mean", "rand256"), ("max", "rand256"),
                           ("max", None), ("min", "ramp2"), ("min", None), ("mean", "n255"),
                           ("max", "rand256")):
            pkg.set_projection(mode)
            set_table(pkg, name)
            with torch.cuda.stream(stream) if own_stream else torch.cuda.stream(None):
                frames.append((mode, name, render(pkg, torch, W, H, camera("C1"), method=13)))
        for mode, name, got in frames:
            assert_same(got, reference(DIMS, 8, "f32", "C1", W, H, name, "combine", mode),
                        f"{mode} {name}")
        assert_same(frames[2][2], frames[0][2], "max again")
        assert not np.array_equal(frames[1][2][0], frames[0][2][0])
        # back on the default stream after frames on another one
        pkg.set_stream(None)
        pkg.set_projection("mean")
        set_table(pkg, None)
        got = render(pkg, torch, W, H, camera("C1"), method=10)
        assert_same(got, reference(DIMS, 8, "f32", "C1", W, H, None, "trilinear", "mean"),
                    "default stream")
    finally:
        torch.cuda.synchronize()
        pkg.set_stream(None)


def test_lifetime(pkg, gpu):
    import torch
    upload_F_planes(pkg, DIMS, 8, "f32")
    planes = (pkg.weighted_info(), pkg.crossing_info())
    before = pkg.layout_info()["resident_bytes"]
    pkg.set_projection("max")
    assert (pkg.weighted_info(), pkg.crossing_info()) == planes  # setting drops no plane
    want = reference(DIMS, 8, "f32", "C1", W, H, None, "combine", "max")
    assert_same(render(pkg, torch, W, H, camera("C1"), method=13), want, "first")
    # freeCudaBuffers frees the table's device copy and every plane; the mode stays set
    pkg.freeCudaBuffers()
    assert pkg.projection() == "max"
    assert pkg.crossing_info() == (None, 0)
    upload_F_planes(pkg, DIMS, 8, "f32")
    assert_same(render(pkg, torch, W, H, camera("C1"), method=13), want, "after freeCudaBuffers")
    # a new volume, vr_convert_f16 and the releases keep it too
    pkg.convert_f16()
    pkg.release_crossing()
    pkg.release_stats()
    assert pkg.projection() == "max"
    pkg.bake_crossing()
    assert_same(render(pkg, torch, W, H, camera("C1"), method=13),
                reference(DIMS, 8, "f16", "C1", W, H, None, "combine", "max"),
                "after vr_convert_f16")
    assert pkg.layout_info()["resident_bytes"] == before


# ---- 8. refusals ----

def test_refusals(pkg, orc, gpu):
    """with a projection set nothing falls back to compositing: what has no plane march
    is VR_ERR_UNSUPPORTED, and succeeds as before once the projection is cleared"""
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
        pkg.set_projection("max")
        for k, f in calls.items():
            with pytest.raises(pkg.VRError) as e:
                f()
            assert e.value.status == lib.VR_ERR_UNSUPPORTED, k
            msg = str(e.value)
            assert "maximum projection" in msg and "bake" in msg, (k, msg)
            assert "vr_set_projection(0)" in msg, (k, msg)
        # a 2-D table at the same time: refused even with both planes resident
        pkg.bake_weighted()
        pkg.set_transfer_function_2d(np.zeros((2, 2, 4), np.float32), 10)
        with pytest.raises(pkg.VRError) as e:
            render(pkg, torch, W, H, m, method=10)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
        assert "classifies one plane" in str(e.value), str(e.value)
        pkg.set_transfer_function_2d(None)
        pkg.release_weighted()
        pkg.set_query_range(0.0, THETA, 8)
        pkg.set_projection(None)
        for k, f in calls.items():
            after = f()
            if isinstance(after, tuple):
                assert_same(after, before[k], k)
            else:
                assert np.array_equal(after, before[k]), k
    finally:
        pkg.set_projection(None)
        pkg.set_transfer_function_2d(None)
        pkg.free_gmm()
