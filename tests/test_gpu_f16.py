"""GPU parity of f16 record volumes (vr_half.hip).

f16 -> f32 widening is exact, so the bar is the project's, unchanged: an f16
volume renders like the CPU oracle fed the same records widened to float32 --
packed RGBA8 identical, samples per pixel identical, float RGBA within 1e-4.
"""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_parity import assert_parity, gpu_render
from test_gpu_random import draw_params

pytestmark = pytest.mark.gpu

DIMS = (24, 20, 16)
SIZES = {"C0": (96, 72), "C1": (88, 60)}
_state = {}


def camera(pkg, cam):
    return pkg.camera.single_test_inv_view() if cam == "C0" else pkg.camera.display_inv_view()


@functools.lru_cache(maxsize=None)
def vol16(dims, nb):
    v = _state["orc"].synth_volume(*dims, nb).astype(np.float16)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def reference(dims, nb, cam, W, H, method, m7=None):
    """the oracle's frame of the widened records, computed once per case"""
    orc, pkg = _state["orc"], _state["pkg"]
    p = orc.make_params(W, H, camera(pkg, cam), query_method=method, m7_dims=m7 or dims)
    return orc.render(vol16(dims, nb).astype(np.float32), p)[:3]


@pytest.fixture(autouse=True)
def _handles(pkg, orc, gpu):
    _state["orc"], _state["pkg"] = orc, pkg
    yield
    pkg.release_stats()


def subnormals(v16):
    bits = v16.view(np.uint16)
    return int(np.sum(((bits & 0x7C00) == 0) & ((bits & 0x03FF) != 0)))


def d2h(ptr, n, dtype):
    import torch
    out = np.zeros(n, dtype)
    torch.cuda.synchronize()
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr),
                         ctypes.c_size_t(out.nbytes), 2) == 0
    return out


def resident_records(pkg, dtype):
    """the resident volume as (nz, ny, nx, B), pitch padding excluded"""
    (nx, ny, nz), b, ptr = pkg.volume_info()
    sy, sz = pkg.volume_layout()
    flat = d2h(ptr, sz * nz * b, dtype)
    return np.stack([flat[z * sz * b:(z * sz + ny * sy) * b].reshape(ny, sy, b)[:, :nx]
                     for z in range(nz)])


@pytest.mark.parametrize("method", [1, 2, 3])
@pytest.mark.parametrize("cam", ["C0", "C1"])
@pytest.mark.parametrize("nb", [1, 2, 4, 8, 16, 32])
def test_f16_matches_oracle_of_widened_records(pkg, orc, gpu, nb, cam, method):
    import torch
    v = vol16(DIMS, nb)
    assert subnormals(v) >= 1, "the data must exercise the widening's subnormal path"
    W, H = SIZES[cam]
    got = gpu_render(pkg, v, W, H, camera(pkg, cam), method, torch)
    assert pkg.volume_dtype() == "f16"
    assert pkg.last_kernel().startswith("k_march_pipe_h<"), pkg.last_kernel()
    assert_parity(got, reference(DIMS, nb, cam, W, H, method), f"f16 x{nb} {cam} m{method}")


def test_f16_frame_differs_from_fp32_frame(pkg, orc, gpu):
    """the parity test discriminates: a build that silently kept the float32 records
    would render the unrounded volume's frame, which is another frame"""
    import torch
    W, H = SIZES["C0"]
    m = camera(pkg, "C0")
    full = orc.render(orc.synth_volume(*DIMS, 8), orc.make_params(W, H, m, query_method=2))[0]
    got = gpu_render(pkg, vol16(DIMS, 8), W, H, m, 2, torch)
    assert_parity(got, reference(DIMS, 8, "C0", W, H, 2), "f16 x8 C0 m2")
    diff = int(np.sum(got[0] != full))
    print(f"RGBA8 pixels differing from the unrounded float32 frame: {diff}")
    assert diff >= 1


@pytest.mark.parametrize("nb", [1, 8])
def test_f16_awkward_shapes(pkg, orc, gpu, nb):
    """odd-sized volume, eye inside it, ragged and 1 x 1 images, non-default
    density / brightness / transfer offset and scale"""
    import torch
    dims = (13, 7, 5)
    v = vol16(dims, nb)
    wide = v.astype(np.float32)
    m = pkg.camera.display_inv_view((0.0, 0.0), translation=(0.1, -0.2, -0.3))
    rng = np.random.default_rng(1600 + nb)
    pkg.init_distribution(v)
    for W, H in [(70, 13), (1, 1)]:
        for method in (1, 2, 3):
            prm = draw_params(rng)
            got = gpu_render(pkg, None, W, H, m, method, torch, **prm)
            ref = orc.render(wide, orc.make_params(
                W, H, m, density=prm["density"], brightness=prm["brightness"],
                transfer_offset=prm["toff"], transfer_scale=prm["tscale"],
                query_method=method))[:3]
            assert pkg.last_kernel().startswith("k_march_pipe_h<"), pkg.last_kernel()
            assert_parity(got, ref, f"f16 {dims}x{nb} {W}x{H} m{method} {prm}")


@pytest.mark.parametrize("nb", [8, 32])
def test_f16_tile_lists(pkg, orc, gpu, nb):
    """a 3-rank split rendered into poisoned packed buffers and unscattered"""
    import torch
    W, H = SIZES["C1"]
    m = camera(pkg, "C1")
    pkg.init_distribution(vol16(DIMS, nb))
    lists = pkg.tiles.tile_lists(W, H, 3, m)
    n_slots = lists.shape[1]
    dl = torch.from_numpy(lists.view(np.int32).copy()).cuda()
    packed = torch.full((3, n_slots * 256), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    for r in range(3):
        pkg.render(pkg.make_desc(packed[r], W, H, m, query_method=1, d_tile_list=dl[r],
                                 n_tiles=n_slots))
        assert pkg.last_kernel().startswith("k_march_pipe_h<"), pkg.last_kernel()
    frame = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    pkg.unscatter_tiles(packed, dl, 3, n_slots, frame, W, H)
    torch.cuda.synchronize()
    ref8 = reference(DIMS, nb, "C1", W, H, 1)[0]
    assert np.array_equal(frame.cpu().numpy().view(np.uint32).reshape(H, W), ref8)


def midpoint_volume():
    """for every f16 value h in [0, 1): the float32 midpoint of h and its successor
    and that midpoint's two float32 neighbours -- ties to even and the values just
    off them, through the subnormal / normal boundary; 3 x 15360 = 48 x 32 x 30"""
    h = np.arange(0, 0x3C00, dtype=np.uint16)
    lo = h.view(np.float16).astype(np.float32)
    hi = (h + np.uint16(1)).view(np.float16).astype(np.float32)
    mid = (lo + hi) * np.float32(0.5)  # exact: 12 significant bits
    below = np.nextafter(mid, np.float32(-1.0))
    above = np.nextafter(mid, np.float32(2.0))
    v = np.stack([below, mid, above], axis=1).astype(np.float32)
    assert v.size == 48 * 32 * 30
    return v.reshape(30, 32, 48, 1)


def test_convert_f16(pkg, orc, gpu):
    import torch
    vol = orc.synth_volume(*DIMS, 8)
    pkg.init_distribution(vol)
    assert pkg.volume_dtype() == "f32"
    pkg.convert_f16()
    assert pkg.volume_dtype() == "f16"
    got = resident_records(pkg, np.uint16)
    assert np.array_equal(got, vol.astype(np.float16).view(np.uint16))
    with pytest.raises(pkg.VRError) as e:
        pkg.convert_f16()
    assert e.value.status == pkg._lib.VR_ERR_STATE
    # a frame after the conversion = a frame after a direct f16 upload
    W, H = SIZES["C1"]
    m = camera(pkg, "C1")
    a = gpu_render(pkg, None, W, H, m, 2, torch)
    assert pkg.last_kernel().startswith("k_march_pipe_h<"), pkg.last_kernel()
    b = gpu_render(pkg, vol16(DIMS, 8), W, H, m, 2, torch)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert_parity(a, reference(DIMS, 8, "C1", W, H, 2), "converted x8 C1 m2")
    # ties to even, subnormals kept
    mv = midpoint_volume()
    pkg.init_distribution(mv)
    pkg.convert_f16()
    got = resident_records(pkg, np.uint16)
    want = mv.astype(np.float16).view(np.uint16)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, (bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


def test_f16_baked_statistics(pkg, orc, gpu):
    import torch
    for cam in ("C0", "C1"):
        W, H = SIZES[cam]
        m = camera(pkg, cam)
        pkg.init_distribution(vol16(DIMS, 8))
        with pytest.raises(pkg.VRError) as e:  # unbaked method 7: no f16 march
            gpu_render(pkg, None, W, H, m, 7, torch)
        assert e.value.status == pkg._lib.VR_ERR_UNSUPPORTED
        assert "basicDataProcessing" in str(e.value)
        pkg.bake_stats()
        for method in (1, 2, 3):
            got = gpu_render(pkg, None, W, H, m, method, torch)
            assert not pkg.last_kernel().startswith("k_march_pipe_h<"), pkg.last_kernel()
            assert_parity(got, reference(DIMS, 8, cam, W, H, method), f"baked f16 {cam} m{method}")
        for grid in (DIMS, (10, 12, 20)):
            got = gpu_render(pkg, None, W, H, m, 7, torch, m7=grid)
            assert_parity(got, reference(DIMS, 8, cam, W, H, 7, grid),
                          f"baked f16 {cam} m7 grid {grid}")
        pkg.release_stats()
        for method in (1, 2, 3):
            got = gpu_render(pkg, None, W, H, m, method, torch)
            assert pkg.last_kernel().startswith("k_march_pipe_h<"), pkg.last_kernel()
            assert_parity(got, reference(DIMS, 8, cam, W, H, method), f"f16 {cam} m{method}")


@pytest.mark.parametrize("cam", ["C0", "C1"])
@pytest.mark.parametrize("nb", [4, 8])
def test_f16_footprint(pkg, orc, gpu, nb, cam):
    import torch
    W, H = SIZES[cam]
    m = camera(pkg, cam)
    v = vol16(DIMS, nb)
    pkg.init_distribution(v)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    for method in (1, 2, 3):
        d = pkg.make_desc(out, W, H, m, query_method=method)
        u = pkg.count_footprint(d)
        ref = orc.count_footprint(v.astype(np.float32),
                                  orc.make_params(W, H, m, query_method=method))
        assert u == ref, f"x{nb} {cam} m{method}: U {u} != oracle {ref}"
        assert pkg.footprint_bytes(d) == u * nb * 2


def test_f16_argument_checks(pkg, orc, gpu):
    import torch
    with pytest.raises(pkg.VRError) as e:
        pkg.init_distribution(orc.synth_volume(6, 5, 4, 3).astype(np.float16))
    assert e.value.status == pkg._lib.VR_ERR_UNSUPPORTED
    # an adopted buffer at an odd element offset: 2-byte aligned, 16 needed
    v = vol16(DIMS, 8)
    buf = torch.zeros(v.size + 8, dtype=torch.float16, device="cuda")
    t = buf[1:1 + v.size].view(*v.shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == 2
    with pytest.raises(pkg.VRError) as e:
        pkg.init_distribution(t, adopt=True)
    assert e.value.status == pkg._lib.VR_ERR_ARG
    # the aligned buffer is adopted, and copied, as f16
    buf[:v.size] = torch.from_numpy(np.array(v)).cuda().reshape(-1)
    t = buf[:v.size].view(*v.shape)
    W, H = SIZES["C0"]
    m = camera(pkg, "C0")
    for adopt in (True, False):
        pkg.init_distribution(t, adopt=adopt)
        assert pkg.volume_dtype() == "f16"
        got = gpu_render(pkg, None, W, H, m, 1, torch)
        assert_parity(got, reference(DIMS, 8, "C0", W, H, 1), f"torch f16 adopt={adopt}")
    # a float32 upload after an f16 volume: float32 again, on the existing kernels
    vol = orc.synth_volume(*DIMS, 8)
    got = gpu_render(pkg, vol, W, H, m, 1, torch)
    assert pkg.volume_dtype() == "f32"
    assert not pkg.last_kernel().startswith("k_march_pipe_h<"), pkg.last_kernel()
    assert_parity(got, orc.render(vol, orc.make_params(W, H, m, query_method=1))[:3],
                  "float32 after f16")
