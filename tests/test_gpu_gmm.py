"""GPU parity of the GMM march (config 5) against the CPU
oracle, through the C-ABI: whole-volume renders, slab chains with only each
slab's slices resident, the on-device generator, the footprint count and the
error paths.  Bar: packed RGBA8 and samples per pixel identical, float RGBA
within 1e-4 (the north star's tolerance; the decode order is fixed, so the
results are in fact bit-identical: tests/test_gpu_bitparity.py::test_gmm asserts
that, word for word, on frames that magnify the decode)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4


def gmm_render(pkg, W, H, m, method, torch, slab=None, density=0.05):
    out = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(H * W * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((H * W,), -2, dtype=torch.int32, device="cuda")
    d = pkg.make_desc(out, W, H, m, query_method=method, density=density, volume_size=(1, 1, 1),
                      d_output_f=out_f, d_steps=steps)
    pkg.render_gmm(d, slab)
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint32).reshape(H, W),
            out_f.cpu().numpy().reshape(H, W, 4), steps.cpu().numpy().reshape(H, W))


def check(got, ref, what):
    g8, gf, gn = got
    assert np.array_equal(gn, ref["out_n"]), f"{what}: samples per pixel differ"
    assert np.array_equal(g8, ref["out"]), f"{what}: {int(np.sum(g8 != ref['out']))} RGBA8 differ"
    err = float(np.max(np.abs(gf - ref["out_f"])))
    assert err <= TOL, f"{what}: max |RGBA - oracle| = {err}"


CAMS = {"C0": None, "C1": (30.0, 45.0), "below": (180.0, 0.0), "side": (90.0, 0.0)}


def cam(pkg, name):
    return pkg.camera.single_test_inv_view() if CAMS[name] is None else \
        pkg.camera.display_inv_view(CAMS[name])


@pytest.mark.parametrize("K", [8, 16, 32])
@pytest.mark.parametrize("method", [1, 2])
def test_gmm_whole_volume(pkg, orc, gpu, K, method):
    import torch
    dims = (26, 22, 18)
    wm, sg = orc.synth_gmm(*dims, K, seed=K)
    pkg.init_gmm(wm, sg)
    for c in CAMS:
        for density in (0.05, 0.6):
            m = cam(pkg, c)
            got = gmm_render(pkg, 80, 64, m, method, torch, density=density)
            ref = orc.render_gmm(wm, sg, dims, orc.make_params(80, 64, m, query_method=method,
                                                               density=density))
            check(got, ref, f"K={K} m{method} {c} d={density}")
    assert pkg.last_kernel().startswith("k_march_gmm") and f"<B={K},M={method}>" in pkg.last_kernel()
    pkg.free_gmm()


def test_synth_gmm_matches_oracle(pkg, orc, gpu):
    import torch
    dims = (20, 14, 12)
    for zb, ns in ((0, 12), (5, 4)):
        pkg.synthesize_gmm(dims, 16, seed=99, z_base=zb, nslices=ns)
        (X, Y, Z), K, z0, n, pwm, psg = pkg.gmm_info()
        assert (X, Y, Z, K, z0, n) == (20, 14, 12, 16, zb, ns)
        nvox = 20 * 14 * ns
        wm = torch.empty(nvox * K * 2, dtype=torch.float32, device="cuda")
        sg = torch.empty(nvox * K, dtype=torch.float32, device="cuda")
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert hip.hipMemcpy(wm.data_ptr(), pwm, wm.numel() * 4, 3) == 0
        assert hip.hipMemcpy(sg.data_ptr(), psg, sg.numel() * 4, 3) == 0
        rwm, rsg = orc.synth_gmm(*dims, 16, seed=99, z_base=zb, nslices=ns)
        assert np.array_equal(wm.cpu().numpy(), rwm.reshape(-1))
        assert np.array_equal(sg.cpu().numpy(), rsg.reshape(-1))
    pkg.free_gmm()


@pytest.mark.parametrize("c,nslabs,K", [(c, n, 16) for c in ("C0", "C1", "below") for n in (2, 3, 5)]
                         + [("C1", 3, 8), ("C0", 2, 8), ("C1", 3, 32), ("below", 5, 32)])
def test_gmm_slab_chain(pkg, orc, gpu, c, nslabs, K):
    """each slab generated on its own (only its slices + halo resident), the alive
    list handed from slab to slab on the device: the frame, the samples and every
    alive ray's exact state (9-word entries, written by the K/4 lanes of a ray's
    group: 2 lanes at K = 8) equal the oracle's chain and the whole-volume render"""
    import torch
    dims = (24, 20, 23)
    method, W, H = 1 if nslabs != 3 else 2, 72, 56
    m = cam(pkg, c)
    direction = pkg.slabs.march_direction(m, W, H)
    bounds = pkg.slabs.slab_bounds(dims[2], nslabs, direction)
    wm, sg = orc.synth_gmm(*dims, K)
    p = orc.make_params(W, H, m, query_method=method, density=0.2)
    full = orc.render_gmm(wm, sg, dims, p)
    out = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(H * W * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((H * W,), -2, dtype=torch.int32, device="cuda")
    d = pkg.make_desc(out, W, H, m, query_method=method, density=0.2, volume_size=(1, 1, 1),
                      d_output_f=out_f, d_steps=steps)
    bufs = [torch.zeros((W * H, pkg.slabs.RAY_WORDS), dtype=torch.int32, device="cuda") for _ in range(2)]
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    n_in = 0
    ref_rays = None
    for i, (z_lo, z_hi) in enumerate(bounds):
        zb, ns = pkg.slabs.resident_slices(z_lo, z_hi, dims[2])
        pkg.synthesize_gmm(dims, K, z_base=zb, nslices=ns)
        rin = bufs[(i + 1) % 2] if i else None
        s = pkg.gmm_slab(z_lo, z_hi, bufs[i % 2], cnt[0:1], d_rays_in=rin, n_rays_in=n_in)
        pkg.render_gmm(d, s)
        torch.cuda.synchronize()
        n_in = int(cnt[0].item())
        r = orc.render_gmm(wm[zb:zb + ns], sg[zb:zb + ns], dims, p, z_base=zb, slab=(z_lo, z_hi),
                           rays_in=ref_rays)
        ref_rays = r["rays_out"]
        assert n_in == ref_rays.shape[0], f"slab {i}: {n_in} alive rays vs {ref_rays.shape[0]}"
        got_rays = bufs[i % 2][:n_in].cpu().numpy().view(np.uint32)
        pix = lambda a: a[:, 8] & 0x7FFFFF  # the entry's last word: pixel | samples << 23
        order = np.argsort(pix(got_rays), kind="stable")
        assert np.array_equal(got_rays[order], ref_rays[np.argsort(pix(ref_rays), kind="stable")])
    assert n_in == 0
    torch.cuda.synchronize()
    got = (out.cpu().numpy().view(np.uint32).reshape(H, W), out_f.cpu().numpy().reshape(H, W, 4),
           steps.cpu().numpy().reshape(H, W))
    check(got, full, f"{nslabs} slabs {c}")
    pkg.free_gmm()


def test_gmm_slab_footprint_and_list_capacity(pkg, orc, gpu):
    """U of every slab of a chain (vr_gmm_count_footprint_slab, what bench.py
    --slab-rehearsal prices each slab's launch with) equals the oracle's count of
    that slab; and the library resets the alive-list counter itself, on its own
    stream, before every slab launch (include/vr.h): a counter the caller left
    at any value counts exactly the rays that leave alive, and no entry lands
    past the list's capacity"""
    import torch
    dims = (24, 20, 23)
    K, W, H = 16, 72, 56
    m = cam(pkg, "C0")
    bounds = pkg.slabs.slab_bounds(dims[2], 3, pkg.slabs.march_direction(m, W, H))
    wm, sg = orc.synth_gmm(*dims, K)
    p = orc.make_params(W, H, m, query_method=1)
    out = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    d = pkg.make_desc(out, W, H, m, query_method=1, volume_size=(1, 1, 1))
    bufs = [torch.zeros((W * H, pkg.slabs.RAY_WORDS), dtype=torch.int32, device="cuda") for _ in range(2)]
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    n_in, ref_rays = 0, None
    for i, (z_lo, z_hi) in enumerate(bounds):
        zb, ns = pkg.slabs.resident_slices(z_lo, z_hi, dims[2])
        pkg.synthesize_gmm(dims, K, z_base=zb, nslices=ns)
        cnt.fill_(W * H - 3)  # stale: the count pass resets it
        s = pkg.gmm_slab(z_lo, z_hi, bufs[i % 2], cnt, d_rays_in=bufs[(i + 1) % 2] if i else None,
                         n_rays_in=n_in)
        u = pkg.gmm_count_footprint(d, s)
        r = orc.render_gmm(wm[zb:zb + ns], sg[zb:zb + ns], dims, p, z_base=zb, slab=(z_lo, z_hi),
                           rays_in=ref_rays, want_mark=True)
        assert u == r["U"] and (u > 0 or i > 0), (i, u, r["U"])
        torch.cuda.synchronize()
        assert int(cnt.item()) == r["rays_out"].shape[0]
        cnt.fill_(0x7FFFFFFF)  # stale: the render resets it
        pkg.render_gmm(d, s)
        torch.cuda.synchronize()
        n_in, ref_rays = int(cnt.item()), r["rays_out"]
        assert n_in == ref_rays.shape[0]
    # capacity: slab 0 from the camera holds at most W*H entries; a counter left
    # at W*H - 3 (by the caller, on its own stream) is reset
    # by the launch: exactly the alive rays are listed, the rows past the list untouched
    zb, ns = pkg.slabs.resident_slices(*bounds[0], dims[2])
    pkg.synthesize_gmm(dims, K, z_base=zb, nslices=ns)
    big = torch.full((W * H + 64, pkg.slabs.RAY_WORDS), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cnt.fill_(W * H - 3)
    pkg.render_gmm(d, pkg.gmm_slab(*bounds[0], big, cnt))
    torch.cuda.synchronize()
    alive = orc.render_gmm(wm[zb:zb + ns], sg[zb:zb + ns], dims, p, z_base=zb,
                           slab=bounds[0])["rays_out"].shape[0]
    assert alive > 3 and int(cnt.item()) == alive
    assert bool((big[W * H:] == 0x5A5A5A5A).all()), "entries written past the list's capacity"
    assert not bool((big[:alive] == 0x5A5A5A5A).all(dim=1).any()), "an alive ray's row unwritten"
    pkg.free_gmm()


def test_gmm_footprint_count(pkg, orc, gpu):
    import torch
    dims = (30, 26, 22)
    wm, sg = orc.synth_gmm(*dims, 16)
    pkg.init_gmm(wm, sg)
    for c in ("C0", "C1"):
        m = cam(pkg, c)
        out = torch.zeros(96 * 80, dtype=torch.int32, device="cuda")
        d = pkg.make_desc(out, 96, 80, m, query_method=1, volume_size=(1, 1, 1))
        u = pkg.gmm_count_footprint(d)
        ref = orc.render_gmm(wm, sg, dims, orc.make_params(96, 80, m, query_method=1),
                             want_mark=True)
        assert u == ref["U"] > 0
    pkg.free_gmm()


def test_gmm_errors(pkg, orc, gpu):
    import torch
    dims = (16, 16, 16)
    pkg.synthesize_gmm(dims, 8, z_base=4, nslices=6)
    out = torch.zeros(32 * 32, dtype=torch.int32, device="cuda")
    rays = torch.zeros((32 * 32, pkg.slabs.RAY_WORDS), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    m = pkg.camera.single_test_inv_view()
    d = pkg.make_desc(out, 32, 32, m, query_method=1, volume_size=(1, 1, 1))
    with pytest.raises(pkg.VRError, match="resident"):
        pkg.render_gmm(d)  # not all slices resident
    with pytest.raises(pkg.VRError, match="needs slices"):
        pkg.render_gmm(d, pkg.gmm_slab(4, 10, rays, cnt))  # halo slice 10 missing
    pkg.render_gmm(d, pkg.gmm_slab(4, 9, rays, cnt))      # [4, 9) + halo 9: resident
    d3 = pkg.make_desc(out, 32, 32, m, query_method=3, volume_size=(1, 1, 1))
    with pytest.raises(pkg.VRError) as e:
        pkg.render_gmm(d3, pkg.gmm_slab(4, 9, rays, cnt))
    assert e.value.status == pkg._lib.VR_ERR_UNSUPPORTED
    side = pkg.make_desc(out, 32, 32, pkg.camera.display_inv_view((90.0, 0.0)), query_method=1,
                         volume_size=(1, 1, 1))
    with pytest.raises(pkg.VRError, match="both directions"):
        pkg.render_gmm(side, pkg.gmm_slab(4, 9, rays, cnt))
    # an alive-list entry holds the pixel in 23 bits: a slab launch of more than
    # 2^23 pixels is refused before anything runs (3840 x 2160 fits; a whole-
    # volume render has no list and no limit)
    big = pkg.make_desc(out, 4096, 2049, m, query_method=1, volume_size=(1, 1, 1))
    with pytest.raises(pkg.VRError, match="2\\^23"):
        pkg.render_gmm(big, pkg.gmm_slab(4, 9, rays, cnt))
    with pytest.raises(pkg.VRError):
        pkg.synthesize_gmm(dims, 12)  # K must be 8, 16 or 32
    torch.cuda.synchronize()
    pkg.free_gmm()


def test_gmm_golden_fixtures(pkg, gpu):
    """the GPU march against the committed GMM fixtures (tests/golden/gmm*.npz), the
    volume generated on the device from the fixture's seed"""
    import glob
    import os
    import torch
    files = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "gmm*.npz")))
    assert len(files) == 4
    for path in files:
        z = np.load(path, allow_pickle=False)
        nx, ny, nz, K = (int(v) for v in z["gmm_dims"])
        pkg.synthesize_gmm((nx, ny, nz), K, seed=int(z["seed"]))
        W, H = (int(v) for v in z["image"])
        got = gmm_render(pkg, W, H, z["inv_view"], int(z["method"]), torch,
                         density=float(z["density"]))
        ref = {"out": z["rgba8"], "out_f": z["rgba_f"], "out_n": z["steps"].astype(np.int32)}
        # out_n: the fixture holds -2 for pixels outside any ray (none here) like the render
        check(got, ref, os.path.basename(path))
    pkg.free_gmm()


@pytest.mark.parametrize("c", ["C0", "below", "C1"])
@pytest.mark.parametrize("S,method", [(1, 1), (4, 2), (7, 1), (40, 2)])
def test_gmm_streamed_slabs(pkg, orc, gpu, c, S, method):
    """host-pinned slabs streamed through a 2-buffer HBM ring (stream.GmmStream): the
    frame equals the oracle's whole-volume render bit for bit, for slabs of 1 slice up
    to one slab (S >= nz), rays marching towards -z and +z"""
    import torch
    dims = (24, 20, 17)
    K = 16
    wm, sg = orc.synth_gmm(*dims, K, seed=3)
    st = pkg.stream.GmmStream(torch.from_numpy(wm.copy()), torch.from_numpy(sg.copy()), S)
    m = cam(pkg, c)
    if pkg.slabs.march_direction(m, 72, 56) == 0:
        pytest.skip("view crosses z both ways")
    W, H = 72, 56
    out = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(H * W * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((H * W,), -2, dtype=torch.int32, device="cuda")
    d = pkg.make_desc(out, W, H, m, query_method=method, volume_size=(1, 1, 1), d_output_f=out_f,
                      d_steps=steps)
    s = torch.cuda.Stream()
    info = st.render(d, s)
    torch.cuda.synchronize()
    assert info["slabs"] == -(-dims[2] // S)
    got = (out.cpu().numpy().view(np.uint32).reshape(H, W), out_f.cpu().numpy().reshape(H, W, 4),
           steps.cpu().numpy().reshape(H, W))
    ref = orc.render_gmm(wm, sg, dims, orc.make_params(W, H, m, query_method=method))
    check(got, ref, f"streamed S={S} m{method} {c}")
    # a second frame reuses the ring (buffers, events) and gives the same image
    first = out.clone()
    out.zero_()
    st.render(d, s)
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    pkg.set_stream(None)


def test_config5_at_size(pkg, orc, gpu):
    """BASELINE config 5 at its size: 2048^3 x 16-component GMM (1.65 TB) at
    3840x2160, C0, method 1, rendered on one GPU as the 8-rank z-slab chain
    renders it -- each rank's slab (its slices + halo, 207 GB) generated in HBM
    in turn, the alive list handed on in HBM -- against the oracle's
    whole-volume render of the whole frame (all 2160 rows), whose records it
    computes from the voxel index as a sample reads them (no host holds the
    volume).  Slabs after the
    one that ends the last ray receive no rays and are not generated."""
    import torch
    n, K, W, H = 2048, 16, 3840, 2160
    pkg.freeCudaBuffers()
    pkg.free_gmm()
    torch.cuda.empty_cache()
    m = pkg.camera.single_test_inv_view()
    direction = pkg.slabs.march_direction(m, W, H)
    bounds = pkg.slabs.slab_bounds(n, 8, direction)
    zb, ns = pkg.slabs.resident_slices(*bounds[0], n)
    need = n * n * ns * K * 12 + 2 * W * H * 48 + (2 << 30)
    free, _ = torch.cuda.mem_get_info()
    assert free >= need, f"{free / 2**30:.0f} GiB free, a slab needs {need / 2**30:.0f}"
    frame = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    steps = torch.full((W * H,), -2, dtype=torch.int32, device="cuda")
    d = pkg.make_desc(frame, W, H, m, query_method=1, volume_size=(1, 1, 1), d_steps=steps)
    bufs = [torch.zeros((W * H, pkg.slabs.RAY_WORDS), dtype=torch.int32, device="cuda") for _ in range(2)]
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    n_in, done = 0, 0
    try:
        for i, (z_lo, z_hi) in enumerate(bounds):
            if i and n_in == 0:
                break
            zb, ns = pkg.slabs.resident_slices(z_lo, z_hi, n)
            pkg.synthesize_gmm((n, n, n), K, 20261015, z_base=zb, nslices=ns)
            pkg.render_gmm(d, pkg.gmm_slab(z_lo, z_hi, bufs[i % 2], cnt,
                                           d_rays_in=bufs[(i + 1) % 2] if i else None,
                                           n_rays_in=n_in))
            torch.cuda.synchronize()
            n_in = int(cnt.item())
            done = i + 1
            print(f"slab {i} z [{z_lo}, {z_hi}): {n_in} rays alive", flush=True)
    finally:
        pkg.free_gmm()
    assert n_in == 0 and done >= 2
    # the whole frame: 8.3 M pixels of oracle in ~40 s on the box's 16 threads
    # (profiles/r06/final_blocks/pytest_config5_full.log); VR_CONFIG5_ROW_STEP=n
    # checks every n-th row only
    step = int(os.environ.get("VR_CONFIG5_ROW_STEP", "1"))
    rows = np.arange(0, H, step, dtype=np.int32)
    ref, ref_n, samples = orc.render_gmm_rows_proc(
        (n, n, n), K, orc.make_params(W, H, m, query_method=1), rows, nthreads=orc.max_threads())
    got = frame.cpu().numpy().view(np.uint32).reshape(H, W)[rows]
    got_n = steps.cpu().numpy().reshape(H, W)[rows]
    assert int(np.sum(ref_n > 0)) > len(rows) * W // 4 and samples > 0
    assert np.array_equal(got_n, ref_n), f"{int(np.sum(got_n != ref_n))} sample counts differ"
    assert np.array_equal(got, ref), f"{int(np.sum(got != ref))} RGBA8 pixels differ"
