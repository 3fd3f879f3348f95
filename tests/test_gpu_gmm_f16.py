"""GPU parity of the f16 GMM march (k_march_gmm_h) against
the CPU oracle fed the same records widened to float32, through the C-ABI:
whole-volume renders, every way of making an f16 volume resident, slab chains,
two slots of two dtypes, streamed slabs, the footprint count and the error
paths.  f16 -> f32 widening is exact and the statistic's evaluation order is
fixed, so the bar is bit identity: packed RGBA8, samples per pixel and float
RGBA all exactly equal."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAMS = {"C0": None, "C1": (30.0, 45.0), "below": (180.0, 0.0), "side": (90.0, 0.0)}


def cam(pkg, name):
    return pkg.camera.single_test_inv_view() if CAMS[name] is None else \
        pkg.camera.display_inv_view(CAMS[name])


@functools.lru_cache(maxsize=None)
def _records(orc, dims, K, seed, z_base=0, nslices=None):
    """(fp32 wm, sg, f16 wm, sg, widened wm, sg) of the synthetic volume; the
    rounding must really change the records"""
    wm, sg = orc.synth_gmm(*dims, K, seed=seed, z_base=z_base, nslices=nslices)
    hwm, hsg = wm.astype(np.float16), sg.astype(np.float16)
    wwm, wsg = hwm.astype(np.float32), hsg.astype(np.float32)
    assert not np.array_equal(wm, wwm) and not np.array_equal(sg, wsg)
    for a in (wm, sg, hwm, hsg, wwm, wsg):
        a.setflags(write=False)
    return wm, sg, hwm, hsg, wwm, wsg


class Frame:
    def __init__(self, pkg, torch, W, H, m, method, density=0.05):
        self.W, self.H = W, H
        self.out = torch.zeros(H * W, dtype=torch.int32, device="cuda")
        self.out_f = torch.zeros(H * W * 4, dtype=torch.float32, device="cuda")
        self.steps = torch.full((H * W,), -2, dtype=torch.int32, device="cuda")
        self.desc = pkg.make_desc(self.out, W, H, m, query_method=method, density=density,
                                  volume_size=(1, 1, 1), d_output_f=self.out_f,
                                  d_steps=self.steps)

    def clear(self):
        self.out.zero_()
        self.out_f.zero_()
        self.steps.fill_(-2)

    def get(self):
        H, W = self.H, self.W
        return (self.out.cpu().numpy().view(np.uint32).reshape(H, W),
                self.out_f.cpu().numpy().reshape(H, W, 4), self.steps.cpu().numpy().reshape(H, W))


def gmm_render(pkg, W, H, m, method, torch, density=0.05):
    f = Frame(pkg, torch, W, H, m, method, density)
    pkg.render_gmm(f.desc)
    torch.cuda.synchronize()
    return f.get()


def check(got, ref, what):
    g8, gf, gn = got
    assert np.array_equal(gn, ref["out_n"]), f"{what}: samples per pixel differ"
    assert np.array_equal(g8, ref["out"]), f"{what}: {int(np.sum(g8 != ref['out']))} RGBA8 differ"
    assert np.array_equal(gf, ref["out_f"]), \
        f"{what}: float RGBA differs, max |d| = {float(np.max(np.abs(gf - ref['out_f'])))}"


def same(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


def read_halves(pkg, torch):
    """the selected slot's planes as the bits the device holds"""
    (X, Y, Z), K, z0, n, pwm, psg = pkg.gmm_info()
    nvox = X * Y * n
    wm = torch.empty(nvox * K * 2, dtype=torch.float16, device="cuda")
    sg = torch.empty(nvox * K, dtype=torch.float16, device="cuda")
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(wm.data_ptr(), pwm, wm.numel() * 2, 3) == 0
    assert hip.hipMemcpy(sg.data_ptr(), psg, sg.numel() * 2, 3) == 0
    return (X, Y, Z, K, z0, n), wm.cpu().numpy().view(np.uint16), sg.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("K", [8, 16, 32])
@pytest.mark.parametrize("method", [1, 2])
def test_gmm_f16_whole_volume(pkg, orc, gpu, K, method):
    import torch
    dims = (26, 22, 18)
    _, _, hwm, hsg, wwm, wsg = _records(orc, dims, K, K)
    pkg.init_gmm(hwm, hsg)
    assert pkg.gmm_dtype() == "f16"
    for c in CAMS:
        for density in (0.05, 0.6):
            m = cam(pkg, c)
            got = gmm_render(pkg, 80, 64, m, method, torch, density=density)
            ref = orc.render_gmm(wwm, wsg, dims, orc.make_params(80, 64, m, query_method=method,
                                                                 density=density))
            check(got, ref, f"K={K} m{method} {c} d={density}")
    assert pkg.last_kernel().startswith("k_march_gmm_h")
    assert f"<B={K},M={method}>" in pkg.last_kernel()
    pkg.free_gmm()


def test_gmm_f16_ways_in_give_one_frame(pkg, orc, gpu):
    """a host float16 array, a copied device tensor and an adopted device tensor"""
    import torch
    dims, K, W, H = (26, 22, 18), 16, 80, 64
    _, _, hwm, hsg, wwm, wsg = _records(orc, dims, K, K)
    m = cam(pkg, "C1")
    ref = orc.render_gmm(wwm, wsg, dims, orc.make_params(W, H, m, query_method=2))
    dwm, dsg = torch.from_numpy(hwm.copy()).cuda(), torch.from_numpy(hsg.copy()).cuda()
    frames = []
    for how in ("host", "copied", "adopted"):
        if how == "host":
            pkg.init_gmm(hwm, hsg)
        else:
            pkg.init_gmm(dwm, dsg, adopt=how == "adopted")
        assert pkg.gmm_dtype() == "f16", how
        frames.append(gmm_render(pkg, W, H, m, 2, torch))
        check(frames[-1], ref, how)
        pkg.free_gmm()
    same(frames[0], frames[1], "copied tensor")
    same(frames[0], frames[2], "adopted tensor")
    assert bool((dwm.cpu() == torch.from_numpy(hwm.copy())).all())  # adopted: not freed, not written


@pytest.mark.parametrize("how", ["convert", "synthesize"])
def test_gmm_f16_planes_are_the_narrowed_generator(pkg, orc, gpu, how):
    """convert_gmm_f16() on a resident fp32 volume and synthesize_gmm(dtype="f16")
    leave the bits of the fp32 generator's values rounded to nearest even"""
    import torch
    dims = (20, 14, 12)
    for zb, ns in ((0, 12), (5, 4)):
        if how == "convert":
            pkg.synthesize_gmm(dims, 16, seed=99, z_base=zb, nslices=ns)
            assert pkg.gmm_dtype() == "f32"
            pkg.convert_gmm_f16()
        else:
            pkg.synthesize_gmm(dims, 16, seed=99, z_base=zb, nslices=ns, dtype="f16")
        assert pkg.gmm_dtype() == "f16"
        shape, wm, sg = read_halves(pkg, torch)
        assert shape == (20, 14, 12, 16, zb, ns)
        _, _, hwm, hsg, _, _ = _records(orc, dims, 16, 99, zb, ns)
        assert np.array_equal(wm, hwm.reshape(-1).view(np.uint16))
        assert np.array_equal(sg, hsg.reshape(-1).view(np.uint16))
    pkg.free_gmm()


@pytest.mark.parametrize("c,nslabs,K", [(c, n, 16) for c in ("C0", "C1", "below") for n in (2, 3, 5)]
                         + [("C1", 3, 8), ("C0", 2, 8), ("C1", 3, 32), ("below", 5, 32)])
def test_gmm_f16_slab_chain(pkg, orc, gpu, c, nslabs, K):
    """each slab synthesized alone as f16 (only its slices + halo resident): after
    every slab the alive count and every 9-word entry equal the oracle's chain on
    the widened records, and the final frame equals the whole-volume render"""
    import torch
    dims = (24, 20, 23)
    method, W, H = 1 if nslabs != 3 else 2, 72, 56
    m = cam(pkg, c)
    direction = pkg.slabs.march_direction(m, W, H)
    bounds = pkg.slabs.slab_bounds(dims[2], nslabs, direction)
    _, _, _, _, wwm, wsg = _records(orc, dims, K, 20261015)
    p = orc.make_params(W, H, m, query_method=method, density=0.2)
    full = orc.render_gmm(wwm, wsg, dims, p)
    f = Frame(pkg, torch, W, H, m, method, density=0.2)
    bufs = [torch.zeros((W * H, pkg.slabs.RAY_WORDS), dtype=torch.int32, device="cuda") for _ in range(2)]
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    n_in = 0
    ref_rays = None
    pix = lambda a: a[:, 8] & 0x7FFFFF  # the entry's last word: pixel | samples << 23
    for i, (z_lo, z_hi) in enumerate(bounds):
        zb, ns = pkg.slabs.resident_slices(z_lo, z_hi, dims[2])
        pkg.synthesize_gmm(dims, K, z_base=zb, nslices=ns, dtype="f16")
        assert pkg.gmm_dtype() == "f16"
        rin = bufs[(i + 1) % 2] if i else None
        s = pkg.gmm_slab(z_lo, z_hi, bufs[i % 2], cnt[0:1], d_rays_in=rin, n_rays_in=n_in)
        pkg.render_gmm(f.desc, s)
        torch.cuda.synchronize()
        n_in = int(cnt[0].item())
        r = orc.render_gmm(wwm[zb:zb + ns], wsg[zb:zb + ns], dims, p, z_base=zb, slab=(z_lo, z_hi),
                           rays_in=ref_rays)
        ref_rays = r["rays_out"]
        assert n_in == ref_rays.shape[0], f"slab {i}: {n_in} alive rays vs {ref_rays.shape[0]}"
        got_rays = bufs[i % 2][:n_in].cpu().numpy().view(np.uint32)
        order = np.argsort(pix(got_rays), kind="stable")
        assert np.array_equal(got_rays[order], ref_rays[np.argsort(pix(ref_rays), kind="stable")])
    assert n_in == 0
    assert pkg.last_kernel().startswith("k_march_gmm_h")
    check(f.get(), full, f"{nslabs} slabs {c}")
    pkg.free_gmm()


def test_gmm_two_slots_two_dtypes(pkg, orc, gpu):
    """fp32 in slot 0 and f16 in slot 1, same seed, both resident: each renders its
    own oracle frame, gmm_dtype() follows gmm_select, freeing one leaves the other"""
    import torch
    dims, K, W, H = (26, 22, 18), 16, 80, 64
    wm, sg, _, _, wwm, wsg = _records(orc, dims, K, K)
    m = cam(pkg, "C0")
    p = orc.make_params(W, H, m, query_method=2)
    ref32 = orc.render_gmm(wm, sg, dims, p)
    ref16 = orc.render_gmm(wwm, wsg, dims, p)
    assert not np.array_equal(ref32["out_f"], ref16["out_f"])
    pkg.gmm_select(0)
    pkg.synthesize_gmm(dims, K, seed=K)
    pkg.gmm_select(1)
    pkg.synthesize_gmm(dims, K, seed=K, dtype="f16")
    try:
        for _ in range(2):
            pkg.gmm_select(0)
            assert pkg.gmm_dtype() == "f32"
            check(gmm_render(pkg, W, H, m, 2, torch), ref32, "slot 0 (f32)")
            assert pkg.last_kernel().startswith("k_march_gmm<")
            pkg.gmm_select(1)
            assert pkg.gmm_dtype() == "f16"
            check(gmm_render(pkg, W, H, m, 2, torch), ref16, "slot 1 (f16)")
            assert pkg.last_kernel().startswith("k_march_gmm_h<")
        pkg.free_gmm()                      # slot 1 goes, slot 0 stays
        with pytest.raises(pkg.VRError) as e:
            pkg.gmm_dtype()
        assert e.value.status == pkg._lib.VR_ERR_STATE
        pkg.gmm_select(0)
        assert pkg.gmm_dtype() == "f32"
        check(gmm_render(pkg, W, H, m, 2, torch), ref32, "slot 0 after freeing slot 1")
        pkg.gmm_select(1)
        pkg.synthesize_gmm(dims, K, seed=K, dtype="f16")
        pkg.gmm_select(0)
        pkg.free_gmm()                      # slot 0 goes, slot 1 stays
        pkg.gmm_select(1)
        check(gmm_render(pkg, W, H, m, 2, torch), ref16, "slot 1 after freeing slot 0")
    finally:
        for slot in (1, 0):
            pkg.gmm_select(slot)
            pkg.free_gmm()


@pytest.mark.parametrize("c", ["C0", "below"])
@pytest.mark.parametrize("S,method", [(1, 1), (4, 2), (40, 2)])
def test_gmm_f16_streamed_slabs(pkg, orc, gpu, c, S, method):
    """GmmStream over float16 host tensors: the frame equals the oracle on the
    widened records, a second frame equals the first, and exactly half the bytes
    of the fp32 stream cross to the device"""
    import torch
    dims, K, W, H = (24, 20, 17), 16, 72, 56
    wm, sg, hwm, hsg, wwm, wsg = _records(orc, dims, K, 3)
    m = cam(pkg, c)
    assert pkg.slabs.march_direction(m, W, H) != 0
    st = pkg.stream.GmmStream(torch.from_numpy(hwm.copy()), torch.from_numpy(hsg.copy()), S)
    assert st.dwm[0].dtype == torch.float16 and st.dsg[1].dtype == torch.float16
    f = Frame(pkg, torch, W, H, m, method)
    s = torch.cuda.Stream()
    try:
        info = st.render(f.desc, s)
        torch.cuda.synchronize()
        assert info["slabs"] == -(-dims[2] // S)
        assert pkg.last_kernel().startswith("k_march_gmm_h")
        first = f.get()
        check(first, orc.render_gmm(wwm, wsg, dims, orc.make_params(W, H, m, query_method=method)),
              f"streamed S={S} m{method} {c}")
        f.clear()
        st.render(f.desc, s)  # a second frame reuses the ring
        torch.cuda.synchronize()
        same(f.get(), first, "second frame")
        st32 = pkg.stream.GmmStream(torch.from_numpy(wm.copy()), torch.from_numpy(sg.copy()), S)
        f.clear()
        info32 = st32.render(f.desc, s)
        torch.cuda.synchronize()
        assert info32["bytes_streamed"] == 2 * info["bytes_streamed"] > 0
        assert st32.slab_bytes == 2 * st.slab_bytes
    finally:
        pkg.set_stream(None)
    with pytest.raises(ValueError, match="same dtype"):
        pkg.stream.GmmStream(torch.from_numpy(hwm.copy()), torch.from_numpy(sg.copy()), S)


def test_gmm_f16_footprint_count(pkg, orc, gpu):
    """gmm_count_footprint, whole and per slab, equals the oracle's U on the
    widened records"""
    import torch
    dims, K, W, H = (24, 20, 23), 16, 72, 56
    _, _, hwm, hsg, wwm, wsg = _records(orc, dims, K, 20261015)
    out = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    pkg.init_gmm(hwm, hsg)
    for c, method in (("C0", 1), ("C1", 2)):
        m = cam(pkg, c)
        d = pkg.make_desc(out, W, H, m, query_method=method, volume_size=(1, 1, 1))
        ref = orc.render_gmm(wwm, wsg, dims, orc.make_params(W, H, m, query_method=method),
                             want_mark=True)
        assert pkg.gmm_count_footprint(d) == ref["U"] > 0
    m = cam(pkg, "C0")
    d = pkg.make_desc(out, W, H, m, query_method=1, volume_size=(1, 1, 1))
    p = orc.make_params(W, H, m, query_method=1)
    bounds = pkg.slabs.slab_bounds(dims[2], 3, pkg.slabs.march_direction(m, W, H))
    bufs = [torch.zeros((W * H, pkg.slabs.RAY_WORDS), dtype=torch.int32, device="cuda") for _ in range(2)]
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    n_in, ref_rays = 0, None
    for i, (z_lo, z_hi) in enumerate(bounds):
        zb, ns = pkg.slabs.resident_slices(z_lo, z_hi, dims[2])
        pkg.init_gmm(hwm[zb:zb + ns], hsg[zb:zb + ns], dims, z_base=zb)
        s = pkg.gmm_slab(z_lo, z_hi, bufs[i % 2], cnt, d_rays_in=bufs[(i + 1) % 2] if i else None,
                         n_rays_in=n_in)
        u = pkg.gmm_count_footprint(d, s)
        r = orc.render_gmm(wwm[zb:zb + ns], wsg[zb:zb + ns], dims, p, z_base=zb, slab=(z_lo, z_hi),
                           rays_in=ref_rays, want_mark=True)
        assert u == r["U"] and (u > 0 or i > 0), (i, u, r["U"])
        torch.cuda.synchronize()
        n_in, ref_rays = int(cnt.item()), r["rays_out"]
        assert n_in == ref_rays.shape[0]
    pkg.free_gmm()


def test_gmm_f16_errors(pkg, orc, gpu):
    import torch
    E = pkg._lib
    pkg.gmm_select(0)
    pkg.free_gmm()
    with pytest.raises(pkg.VRError) as e:
        pkg.convert_gmm_f16()  # nothing resident
    assert e.value.status == E.VR_ERR_STATE
    dims, K = (16, 16, 16), 8
    _, _, hwm, hsg, _, _ = _records(orc, dims, K, 5)
    # an adopted tensor offset by one half: misaligned for the march's loads
    flat_wm = torch.zeros(hwm.size + 8, dtype=torch.float16, device="cuda")
    flat_sg = torch.zeros(hsg.size + 8, dtype=torch.float16, device="cuda")
    ok_wm, ok_sg = flat_wm[8:].view(hwm.shape), flat_sg[8:].view(hsg.shape)
    for wm_off, sg_off in ((1, 8), (8, 1)):
        a = flat_wm[wm_off:wm_off + hwm.size].view(hwm.shape)
        b = flat_sg[sg_off:sg_off + hsg.size].view(hsg.shape)
        with pytest.raises(pkg.VRError) as e:
            pkg.init_gmm(a, b, adopt=True)
        assert e.value.status == E.VR_ERR_ARG
    pkg.init_gmm(ok_wm, ok_sg, adopt=True)  # 16 bytes in: aligned
    pkg.free_gmm()
    # K outside {8, 16, 32}
    with pytest.raises(pkg.VRError) as e:
        pkg.synthesize_gmm(dims, 12, dtype="f16")
    assert e.value.status == E.VR_ERR_UNSUPPORTED
    with pytest.raises(pkg.VRError) as e:
        pkg.init_gmm(np.zeros((4, 4, 4, 12, 2), np.float16), np.zeros((4, 4, 4, 12), np.float16))
    assert e.value.status == E.VR_ERR_UNSUPPORTED
    # mixed dtypes, host and device
    with pytest.raises(ValueError, match="same dtype"):
        pkg.init_gmm(hwm, hsg.astype(np.float32))
    with pytest.raises(ValueError, match="same dtype"):
        pkg.init_gmm(hwm.astype(np.float32), hsg)
    with pytest.raises(ValueError, match="same dtype"):
        pkg.init_gmm(ok_wm, ok_sg.float())
    with pytest.raises(ValueError, match='"f32" or "f16"'):
        pkg.synthesize_gmm(dims, K, dtype="bf16")
    # a slab of an f16 volume: method 3, the missing halo slice, convert twice
    pkg.synthesize_gmm(dims, K, z_base=4, nslices=6, dtype="f16")
    out = torch.zeros(32 * 32, dtype=torch.int32, device="cuda")
    rays = torch.zeros((32 * 32, pkg.slabs.RAY_WORDS), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    m = pkg.camera.single_test_inv_view()
    d = pkg.make_desc(out, 32, 32, m, query_method=1, volume_size=(1, 1, 1))
    with pytest.raises(pkg.VRError, match="needs slices"):
        pkg.render_gmm(d, pkg.gmm_slab(4, 10, rays, cnt))  # halo slice 10 missing
    pkg.render_gmm(d, pkg.gmm_slab(4, 9, rays, cnt))      # [4, 9) + halo 9: resident
    d3 = pkg.make_desc(out, 32, 32, m, query_method=3, volume_size=(1, 1, 1))
    with pytest.raises(pkg.VRError) as e:
        pkg.render_gmm(d3, pkg.gmm_slab(4, 9, rays, cnt))
    assert e.value.status == E.VR_ERR_UNSUPPORTED
    with pytest.raises(pkg.VRError) as e:
        pkg.convert_gmm_f16()  # f16 already
    assert e.value.status == E.VR_ERR_STATE
    pkg.synthesize_gmm(dims, K, z_base=4, nslices=6)
    pkg.convert_gmm_f16()
    with pytest.raises(pkg.VRError) as e:
        pkg.convert_gmm_f16()  # twice
    assert e.value.status == E.VR_ERR_STATE
    torch.cuda.synchronize()
    pkg.free_gmm()
