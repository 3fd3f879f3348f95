"""GPU checks of the gradient-magnitude planes (vr_gradient.hip).

k_bake_grad is float arithmetic in a fixed order which numpy float32 restates bit for
bit (tests/ref_gradient.py), and a frame of a gradient plane is an existing kernel's
frame of one more plane, so every comparison is exact: the whole baked buffer, the
maximum, packed RGBA8, float RGBA and samples per pixel, no tolerance and nothing left
out.  The reference frames are test_gradient.py's, which that file checks on the CPU.
"""
import numpy as np
import pytest

import ref_gradient
from test_crossing import DIMS, H, THETA, W, camera, volume
from test_gpu_crossing import GH, GW, assert_same, gmm_records
from test_gpu_f16 import d2h
from test_gpu_transfer2 import bake_gmm_planes, gmm_frame, kernel_of
from test_gpu_weighted import expected_plane
from test_gradient import (CAMS, FRAMES, G, PLANE_SHAPES, TABLES1, TABLES2, gplane, inv_max,
                           reference, windows)
from test_transfer import RAND256
from test_transfer2 import CODEC, RAMP22, RAND32, codec_records

pytestmark = pytest.mark.gpu

TF_BLEND = "k_march_plane_tf<B=1,M=0>"


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    def clear():
        pkg.set_light(None)
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


def render(pkg, torch, m, method, w=W, h=H, toff=0.0, tscale=1.0):
    """one whole frame of the resident planes"""
    out = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(h * w * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((h * w,), -2, dtype=torch.int32, device="cuda")
    pkg.render(pkg.make_desc(out, w, h, m, query_method=method, transfer_offset=toff,
                             transfer_scale=tscale, volume_size=(1, 1, 1), d_output_f=out_f,
                             d_steps=steps))
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint32).reshape(h, w),
            out_f.cpu().numpy().reshape(h, w, 4), steps.cpu().numpy().reshape(h, w))


def upload_planes(pkg, dims, nb, dtype):
    """records of the oracle's synthetic volume resident with the planes of methods
    1/2/3, 10 (F of [0, THETA)), 11 (the median) and 13 (F) baked"""
    pkg.init_distribution(volume(dims, nb, dtype))
    pkg.set_query_range(0.0, THETA, nb)
    pkg.set_quantile(0.5)
    pkg.set_isovalue(THETA, nb)
    pkg.bake_stats()
    pkg.bake_weighted()
    pkg.bake_quantile()
    pkg.bake_crossing()


def source_plane(pkg, method, dims):
    """the resident plane of `method` as the device holds it: (its floats, (nz, ny, nx))"""
    nx, ny, nz = dims
    if method <= 6:
        (raw, rn), (cod, cn) = pkg.stats_info()
        ptr, n, k = (raw, rn, method - 1) if method <= 3 else (cod, cn, method - 4)
    else:
        ptr, n = {10: pkg.weighted_info, 11: pkg.quantile_info, 13: pkg.crossing_info}[method]()
        k = 0
    assert ptr and n
    flat = d2h(ptr + 4 * n * k, n, np.float32)
    sy = ((nx - 1) // 15 + 1) * 32
    sz = ((ny + 1) // 2) * sy
    assert n == sz * nz
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return flat, flat[z * sz + (y // 2) * sy + (y % 2) * 16 + (x // 15) * 32 + x % 15]


def bricked(stat):
    """test_gpu_weighted.expected_plane without its loop over voxels: stat (nz, ny, nx) in
    the header's brick layout, apron copies included, every other float +0"""
    nz, ny, nx = stat.shape
    sy = ((nx - 1) // 15 + 1) * 32
    sz = ((ny + 1) // 2) * sy
    out = np.zeros(sz * nz, np.float32)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    home = z * sz + (y // 2) * sy + (y % 2) * 16 + (x // 15) * 32 + x % 15
    out[home.ravel()] = stat.ravel()
    ap = (x > 0) & (x % 15 == 0)
    out[home[ap] - 32 + 15] = stat[ap]
    return out


def test_bricked_is_expected_plane():
    s = np.random.default_rng(2704).random((3, 5, 37)).astype(np.float32)
    assert np.array_equal(bricked(s), expected_plane(s))


def check_gradient_plane(pkg, method, dims, what):
    """bakes the gradient plane of `method` and holds the whole buffer -- homes, aprons,
    empty slots and the 4 floats of tail padding -- and the maximum to numpy's"""
    flat, s = source_plane(pkg, method, dims)
    assert pkg.gradient_info(method) == (None, 0, 0.0)
    pkg.bake_gradient(method)
    assert pkg.last_kernel().startswith("k_bake_grad"), pkg.last_kernel()
    ptr, n, mx = pkg.gradient_info(method)
    mag, want_max = ref_gradient.gradient_plane(s)
    want = np.concatenate([bricked(mag), np.zeros(4, np.float32)])
    assert ptr and n == flat.size == want.size - 4, what
    got = d2h(ptr, n + 4, np.float32)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:8], got[bad][:4],
                           want[bad][:4])
    assert np.float32(mx).view(np.uint32) == want_max.view(np.uint32), (what, mx, want_max)
    pkg.bake_gradient(method)  # baked already: nothing changes
    assert pkg.gradient_info(method) == (ptr, n, mx), what
    # the source is untouched
    assert np.array_equal(source_plane(pkg, method, dims)[0].view(np.uint32), flat.view(np.uint32))
    return mag


# ---- 1. plane values ----

@pytest.mark.parametrize("dtype", ("f32", "f16"))
@pytest.mark.parametrize("dims", PLANE_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_plane_values_of_record_volumes(pkg, gpu, dims, dtype):
    """sources 1, 3, 10, 11 and 13.  (1, 1, 1) and (16, 2, 1): x = 15 is both home and
    apron; (15, 1, 3) and (31, 9, 5): x = 30 in two bricks, odd ny; (37, 20, 11): two y
    tiles of a general case; (70, 19, 67): the kernel's tile is 4 bricks -- 60 voxels of
    x -- by 8 y pairs -- 16 rows -- and its z chunk 64 slices, so 2 x 2 tiles and 2
    chunks, the second of 3 slices"""
    upload_planes(pkg, dims, 4, dtype)
    seen = set()
    for method in (1, 3, 10, 11, 13):
        mag = check_gradient_plane(pkg, method, dims, f"{dims} {dtype} method {method}")
        seen.add(mag.tobytes())
    if dims != (1, 1, 1):
        assert len(seen) >= 4  # (10 and 13 hold the same F)
    for method in (1, 3, 10, 11, 13):
        pkg.release_gradient(method)
        assert pkg.gradient_info(method) == (None, 0, 0.0)


@pytest.mark.parametrize("dims", ((16, 2, 1), (37, 20, 11)), ids=lambda d: "x".join(map(str, d)))
def test_plane_values_of_a_codec_volume(pkg, orc, gpu, dims):
    """source 5 of a codec volume: the codec family's dims"""
    pkg.init_codec(*orc.synth_codec(*dims, 8, seed=8))
    pkg.bake_stats()
    check_gradient_plane(pkg, 5, dims, f"codec {dims}")
    with pytest.raises(pkg.VRError) as e:  # no record planes: a state error
        pkg.bake_gradient(1)
    assert e.value.status == pkg._lib.VR_ERR_STATE


# ---- 2. frames ----

def set_frame(pkg, name, dtype):
    """the state of frame `name`; returns (u, toff, tscale, the kernel's name or None)"""
    f = FRAMES[name]
    toff, tscale, voff, vscale = windows(f, dtype)
    for m in (f["u"], f.get("v")):
        if m and m > G:
            pkg.bake_gradient(m - G)
            # the windows come from the library's maximum
            assert float(np.float32(1) / np.float32(pkg.gradient_info(m - G)[2])) == inv_max(
                f["dims"], 8, dtype, m - G)
    kernel = None
    if f["kind"] == "tf1":
        pkg.set_transfer_function(TABLES1[f["table"]])
        kernel = TF_BLEND
    elif f["kind"] == "tf2":
        pkg.set_transfer_function_2d(TABLES2[f["table"]], method_v=f["v"], v_offset=voff,
                                     v_scale=vscale)
        kernel = kernel_of(f["u"], f["v"])
    elif f["kind"] == "proj":
        pkg.set_projection(f["mode"])
        kernel = f"k_march_proj_{f['mode']}<B=1,M=0>"
    elif f["kind"] == "lit":
        pkg.set_transfer_function(TABLES1[f["table"]])
        ka, kd, ks, k = f["light"]
        pkg.set_light(ka, kd, ks, 1 << k)
        kernel = "k_march_lit<B=1,M=0>"
    return f["u"], toff, tscale, kernel


@pytest.mark.parametrize("dtype", ("f32", "f16"))
@pytest.mark.parametrize("name", sorted(n for n in FRAMES if n != "codec"))
def test_frames_against_numpy(pkg, gpu, name, dtype):
    """every frame kind at C0 and C1 through the existing kernel, no layout copy made"""
    import torch
    upload_planes(pkg, DIMS, 8, dtype)
    plain_kernel = {}
    if FRAMES[name]["kind"] == "plain":  # the plane march a record query's plane takes
        for cam in CAMS:
            render(pkg, torch, camera(cam), 10)
            plain_kernel[cam] = pkg.last_kernel()
            assert plain_kernel[cam].startswith("k_march"), plain_kernel
    u, toff, tscale, kernel = set_frame(pkg, name, dtype)
    before = pkg.layout_info()["resident_bytes"]
    for cam in CAMS:
        got = render(pkg, torch, camera(cam), u, toff=toff, tscale=tscale)
        assert pkg.last_kernel() == (kernel or plain_kernel[cam]), (cam, pkg.last_kernel())
        assert_same(got, reference(name, dtype, cam), f"{name} {dtype} {cam}")
    assert pkg.layout_info()["resident_bytes"] == before


def test_codec_pair_against_numpy(pkg, gpu):
    import torch
    pkg.init_codec(*codec_records())
    pkg.bake_stats()
    u, toff, tscale, kernel = set_frame(pkg, "codec", "f32")
    for cam in CAMS:
        got = render(pkg, torch, camera(cam), u, toff=toff, tscale=tscale)
        assert pkg.last_kernel() == kernel
        assert_same(got, reference("codec", "f32", cam), f"codec pair {cam}")
    # and the gradient plane of the codec family as u, under the built-in table
    pkg.set_transfer_function_2d(None)
    got = render(pkg, torch, camera("C1"), G + 6, tscale=inv_max(CODEC, 8, "f32", 6))
    assert (got[2] >= 0).sum() > 1000
    pkg.set_transfer_function(pkg.REFERENCE_TF)
    same = render(pkg, torch, camera("C1"), G + 6, tscale=inv_max(CODEC, 8, "f32", 6))
    assert pkg.last_kernel() == TF_BLEND
    assert_same(got, same, "codec gradient plane: built-in table against REFERENCE_TF")


# ---- 3. life cycle ----

def _refused(pkg, f, what):
    with pytest.raises(pkg.VRError) as e:
        f()
    assert e.value.status == pkg._lib.VR_ERR_UNSUPPORTED, what
    assert "vr_bake_gradient" in str(e.value), (what, str(e.value))


def _bake_all(pkg):
    upload_planes(pkg, DIMS, 8, "f32")
    for m in (1, 2, 10, 11, 13):
        pkg.bake_gradient(m)
        assert pkg.gradient_info(m)[0]


@pytest.mark.parametrize("event", ("set_bin_weights", "release_stats", "init_distribution",
                                   "freeCudaBuffers"))
def test_what_frees_a_source_frees_its_gradient_plane(pkg, gpu, event):
    import torch
    m = camera("C1")
    _bake_all(pkg)
    if event == "set_bin_weights":
        pkg.set_bin_weights(np.arange(8, dtype=np.float32))
        gone, stay = (10,), (1, 2, 11, 13)
    elif event == "release_stats":
        pkg.release_stats()
        gone, stay = (1, 2, 10, 11, 13), ()
    elif event == "init_distribution":
        pkg.init_distribution(volume(DIMS, 8, "f16"))
        gone, stay = (1, 2, 10, 11, 13), ()
    else:
        pkg.freeCudaBuffers()
        gone, stay = (1, 2, 10, 11, 13), ()
    for s in gone:
        assert pkg.gradient_info(s) == (None, 0, 0.0), (event, s)
        _refused(pkg, lambda: render(pkg, torch, m, G + s), f"{event}: frame of {G + s}")
    for s in stay:
        assert pkg.gradient_info(s)[0], (event, s)
        got = render(pkg, torch, m, G + s, tscale=inv_max(DIMS, 8, "f32", s))
        assert (got[2] >= 0).sum() > 1000
    if event == "set_bin_weights":  # a second bake sees the new source
        pkg.bake_weighted()
        mag = check_gradient_plane(pkg, 10, DIMS, "after new weights")
        assert not np.array_equal(mag, gplane(DIMS, 8, "f32", 10)[0])


def test_releasing_a_gradient_plane_leaves_its_source(pkg, gpu):
    import torch
    _bake_all(pkg)
    pkg.set_transfer_function(RAND256)
    before = {s: render(pkg, torch, camera("C1"), s) for s in (1, 10, 13)}
    for s in (1, 10, 13):
        pkg.release_gradient(s)
        assert pkg.gradient_info(s) == (None, 0, 0.0)
        assert pkg.gradient_info(2)[0] and pkg.gradient_info(11)[0]
        assert_same(render(pkg, torch, camera("C1"), s), before[s], f"source {s}")
        _refused(pkg, lambda: render(pkg, torch, camera("C1"), G + s), f"released {s}")


# ---- 4. refusals ----

def test_refusals(pkg, gpu):
    """nothing falls back: a gradient method with no plane, its footprint counts, and
    GMM frames of it are VR_ERR_UNSUPPORTED; each call succeeds as before once the
    cause is cleared"""
    import torch
    lib = pkg._lib
    m = camera("C0")
    upload_planes(pkg, DIMS, 8, "f32")
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")

    def desc(method):
        return pkg.make_desc(out, W, H, m, query_method=method)

    # a per-step gradient method, under every state that serves planes
    for state in ("none", "tf1", "tf2", "proj", "light"):
        if state == "tf1":
            pkg.set_transfer_function(RAND256)
        elif state == "tf2":
            pkg.set_transfer_function_2d(RAMP22, method_v=1)
        elif state == "proj":
            pkg.set_projection("max")
        elif state == "light":
            pkg.set_light(0.3, 0.7, 0.0, 1)
        _refused(pkg, lambda: render(pkg, torch, m, G + 1), f"per step, {state}")
        pkg.set_light(None)
        pkg.set_projection(None)
        pkg.set_transfer_function(None)
        pkg.set_transfer_function_2d(None)
    # v not baked under a 2-D table: the table's refusal, as for any v
    pkg.set_transfer_function_2d(RAMP22, method_v=G + 1)
    with pytest.raises(pkg.VRError) as e:
        render(pkg, torch, m, 1)
    assert e.value.status == lib.VR_ERR_UNSUPPORTED and "bake" in str(e.value)
    pkg.bake_gradient(1)
    got = render(pkg, torch, m, 1)
    assert pkg.last_kernel() == kernel_of(1, G + 1) and (got[2] >= 0).sum() > 1000
    pkg.set_transfer_function_2d(None)
    got = render(pkg, torch, m, G + 1)  # the cause cleared: a frame
    assert (got[2] >= 0).sum() > 1000
    # the footprint counts: never of a gradient method, as before of its source
    pkg.release_stats()
    counts = (pkg.count_footprint(desc(1)), pkg.footprint_bytes(desc(1)))
    pkg.bake_stats()
    for baked in (False, True):
        if baked:
            pkg.bake_gradient(1)
        _refused(pkg, lambda: pkg.count_footprint(desc(G + 1)), f"count, baked {baked}")
        _refused(pkg, lambda: pkg.footprint_bytes(desc(G + 1)), f"bytes, baked {baked}")
    pkg.release_stats()
    assert (pkg.count_footprint(desc(1)), pkg.footprint_bytes(desc(1))) == counts
    # GMM planes have no gradient planes
    bake_gmm_planes(pkg)
    try:
        pkg.free_gmm()
        before = gmm_frame(pkg, torch, m, 1)
        with pytest.raises(pkg.VRError) as e:
            gmm_frame(pkg, torch, m, G + 1)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
        assert_same(gmm_frame(pkg, torch, m, 1), before, "GMM method 1 after a refused u")
        pkg.set_transfer_function_2d(RAND32, method_v=2)
        pair = gmm_frame(pkg, torch, m, 1)
        pkg.set_transfer_function_2d(RAND32, method_v=G + 2)
        with pytest.raises(pkg.VRError) as e:
            gmm_frame(pkg, torch, m, 1)
        assert e.value.status == lib.VR_ERR_UNSUPPORTED
        assert "custom transfer function" in str(e.value)
        pkg.set_transfer_function_2d(RAND32, method_v=2)
        assert_same(gmm_frame(pkg, torch, m, 1), pair, "GMM pair after a refused method_v")
    finally:
        pkg.set_transfer_function_2d(None)
        pkg.release_gmm_stats()
        pkg.release_gmm_range()
        pkg.release_gmm_quantile()
