"""Seeded random parity sweep of the query, f16 and GMM-query marches: what
test_gpu_random.py does for methods 1/2/3/7 on fp32 records, for

  k_march_lin / k_march_quant / k_march_dist / k_march_cross and their baked planes
  (whole frames and multi-rank tile lists), fp32 and f16 records;
  k_march_pipe_h (f16 records, methods 1/2/3) and the f16 bake (methods 1/2/3/7);
  k_march_gmm_h, k_march_gmm_range(_h), k_march_gmm_quant(_h), the GMM planes and
  method 13 on the range plane; slab chains of all of them.

The table marches (k_march_plane_tf, k_march_tf2) have their sweep, from the same
generators module, in tests/test_gpu_random_transfer.py.

Every case is random_cases' dict of its seed: the camera is row-aligned, an exact
quarter turn, inside the volume or oblique, the frame is anything from 1 x 1, the
density runs from rays that cross the volume unsaturated to rays that end within
six samples, and the transfer window moves with the statistic.  Each bar is the
feature's own: the queries are bit-identical to their numpy references (packed
RGBA8, float RGBA and samples per pixel np.array_equal; f16 records against the
reference of the widened records), the f16 record marches and the GMM mean and
variance meet the oracle as test_gpu_parity.assert_parity and test_gpu_gmm.check
ask (RGBA8 and samples identical, float RGBA within 1e-4).  tests/test_random_cases.py
checks on the CPU that the reference frames are worth comparing.  A failure
message carries the seed and the whole case.
"""
import math
import time

import numpy as np
import pytest

import random_cases as rc
import ref_weighted
import test_gpu_gmm
import test_gpu_gmm_f16
from test_gpu_parity import assert_parity, gpu_render
from test_random_cases import (camera, f16_reference, gmm_records, gmm_reference, hist_reference,
                               hist_reference_by_plane, hist_volume, make_case, oracle_params)

pytestmark = pytest.mark.gpu

MARCH = {10: "k_march_lin", 11: "k_march_quant", 12: "k_march_dist", 13: "k_march_cross"}
PLANE_KERNEL = "k_march_cross_plane<B=1,M=13>"


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    """no query state, no planes, no tuning knob and no GMM volume, before and after"""
    def drop():
        pkg.clear_tuning()
        pkg.set_crossing_weights(None)
        pkg.set_query_target(None)
        pkg.set_quantile(None)
        pkg.set_bin_weights(None)
        pkg.release_stats()
        pkg.clear_gmm_range()
        pkg.release_gmm_stats()
        for slot in (1, 0):
            pkg.gmm_select(slot)
            pkg.free_gmm()
    drop()
    yield
    drop()


def set_knobs(tune, case):
    for k, v in case["knobs"].items():
        tune.set(k, v)


def report(case, kernels, t0):
    """one line per case (pytest -s / -rA shows it): the kernels it launched and its
    wall time, reference included"""
    names = "+".join(sorted(kernels)) if not isinstance(kernels, str) else kernels
    print(f"\nCASE {case['sweep']} seed {case['seed']} kernel {names} "
          f"seconds {time.perf_counter() - t0:.2f}")


# ---- histogram queries ----

def set_query(pkg, case):
    q, nb = case["query"], case["nb"]
    if q["state"] == "weights":
        pkg.set_bin_weights(ref_weighted.seeded_weights(nb, seed=q["wseed"]))
    elif q["state"] == "range":
        pkg.set_query_range(q["lo"], q["hi"], nb)
    elif q["state"] == "q":
        pkg.set_quantile(q["q"])
    elif q["state"] == "spread":
        pkg.set_quantile_spread(q["lo"], q["hi"])
    elif q["state"] == "target":
        pkg.set_query_target(np.array(q["target"], np.float32), q["metric"], q["similarity"])
    elif q["state"] == "region":
        pkg.set_query_target_region(q["lo"], q["hi"], metric=q["metric"],
                                    similarity=q["similarity"])
    else:
        pkg.set_isovalue(q["theta"], nb)


def bake_query(pkg, method):
    {10: pkg.bake_weighted, 11: pkg.bake_quantile, 12: pkg.bake_distance,
     13: pkg.bake_crossing}[method]()


def desc_kw(case):
    p = case["params"]
    return dict(density=p["density"], brightness=p["brightness"], transfer_offset=p["toff"],
                transfer_scale=p["tscale"], query_method=case["method"])


def render_frame(pkg, torch, case, m, call=None, **kw):
    """one whole frame of the case: (RGBA8, float RGBA, samples per pixel)"""
    W, H = case["W"], case["H"]
    out = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(H * W * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((H * W,), -2, dtype=torch.int32, device="cuda")
    (call or pkg.render)(pkg.make_desc(out, W, H, m, d_output_f=out_f, d_steps=steps,
                                       **desc_kw(case), **kw))
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint32).reshape(H, W),
            out_f.cpu().numpy().reshape(H, W, 4), steps.cpu().numpy().reshape(H, W))


def assert_same(got, ref, what):
    for name, g, r in zip(("RGBA8", "float RGBA", "samples per pixel"), got, ref):
        assert g.shape == r.shape, f"{what}: {name} shape"
        assert np.array_equal(g, r), f"{what}: {int(np.sum(g != r))} {name} values differ"


def assert_query_kernel(pkg, case, what):
    k = pkg.last_kernel()
    own = f"{MARCH[case['method']]}<B={case['nb']},M={case['method']}>"
    if case["baked"]:
        assert not k.startswith(MARCH[case["method"]] + "<"), f"{what}: baked, yet {k}"
        assert k == PLANE_KERNEL or k.endswith("<B=1,M=0>"), f"{what}: {k}"
    else:
        assert k == own, f"{what}: {k} for {own}"


@pytest.mark.parametrize("seed", range(rc.SWEEPS["hist"][1]))
def test_random_histogram_query_case(pkg, orc, gpu, tune, seed):
    import torch
    t0 = time.perf_counter()
    case = rc.hist_query_case(seed)
    what = f"seed {seed}: {case}"
    m = camera(pkg, case)
    set_knobs(tune, case)
    vol = hist_volume(orc, case)
    pkg.init_distribution(vol)
    assert pkg.volume_dtype() == case["dtype"], what
    if not case["supported"]:
        # 3, 5, 7 and 31 bins: records only methods 1/2/3/7 march; the query is refused
        with pytest.raises(pkg.VRError) as e:
            set_query(pkg, case)
            if case["baked"]:
                bake_query(pkg, case["method"])
            render_frame(pkg, torch, case, m)
        assert e.value.status == pkg._lib.VR_ERR_UNSUPPORTED, what
        report(case, "refused", t0)
        return
    set_query(pkg, case)
    if case["baked"]:
        bake_query(pkg, case["method"])
    got = render_frame(pkg, torch, case, m)
    assert_query_kernel(pkg, case, what)
    kernel = pkg.last_kernel()
    assert_same(got, hist_reference(pkg, case, vol, m), f"{what} kernel {kernel}")
    report(case, kernel, t0)


@pytest.mark.parametrize("seed", range(rc.SWEEPS["tiles"][1]))
def test_random_query_tile_list_case(pkg, orc, gpu, tune, seed):
    """a multi-GPU split of a random query frame: every rank's tile list rendered by
    the query's march or from its plane, the packed slots assembled by k_unscatter,
    equals the reference frame"""
    import torch
    t0 = time.perf_counter()
    case = rc.hist_tile_case(seed)
    what = f"seed {seed}: {case}"
    W, H, world = case["W"], case["H"], case["world"]
    m = camera(pkg, case)
    set_knobs(tune, case)
    vol = hist_volume(orc, case)
    pkg.init_distribution(vol)
    set_query(pkg, case)
    if case["baked"]:
        bake_query(pkg, case["method"])
    lists = pkg.tiles.tile_lists(W, H, world, m)
    n_slots = lists.shape[1]
    packed = torch.full((world, n_slots * 256), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dl = torch.from_numpy(lists.view(np.int32).copy()).cuda()
    kernels = set()
    for r in range(world):
        pkg.render(pkg.make_desc(packed[r], W, H, m, d_tile_list=dl[r], n_tiles=n_slots,
                                 **desc_kw(case)))
        assert_query_kernel(pkg, case, what)
        kernels.add(pkg.last_kernel())
    frame = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    pkg.unscatter_tiles(packed, dl, world, n_slots, frame, W, H)
    torch.cuda.synchronize()
    got = frame.cpu().numpy().view(np.uint32).reshape(H, W)
    ref = hist_reference_by_plane(pkg, case, vol, m)[0]
    assert np.array_equal(got, ref), \
        f"{what} {sorted(kernels)}: {int(np.sum(got != ref))} pixels differ"
    report(case, kernels, t0)


# ---- f16 record marches ----

@pytest.mark.parametrize("seed", range(rc.SWEEPS["f16"][1]))
def test_random_f16_case(pkg, orc, gpu, tune, seed):
    import torch
    t0 = time.perf_counter()
    case = rc.f16_case(seed)
    what = f"seed {seed}: {case}"
    m = camera(pkg, case)
    set_knobs(tune, case)
    vol = hist_volume(orc, case)
    pkg.init_distribution(vol)
    assert pkg.volume_dtype() == "f16", what
    if case["baked"]:
        pkg.bake_stats()
    got = gpu_render(pkg, None, case["W"], case["H"], m, case["method"], torch,
                     m7=case["m7"] if case["method"] == 7 else None, **case["params"])
    kernel = pkg.last_kernel()
    assert kernel.startswith("k_march_pipe_h<") != case["baked"], f"{what}: {kernel}"
    assert_parity(got, f16_reference(orc, case, vol, m), f"{what} kernel {kernel}")
    report(case, kernel, t0)


# ---- GMM volumes ----

def set_gmm_query(pkg, case):
    q = case["query"]
    if case["what"] == "range":
        pkg.set_gmm_range(q["lo"], q["hi"])
    elif case["what"] == "crossing":
        pkg.set_gmm_range(-math.inf, q["theta"])
    elif case["what"] == "quantile":
        if q["state"] == "spread":
            pkg.set_quantile_spread(q["lo"], q["hi"])
        else:
            pkg.set_quantile(q["q"])


def gmm_march_name(case):
    stem = {"mean": "k_march_gmm", "variance": "k_march_gmm", "range": "k_march_gmm_range",
            "quantile": "k_march_gmm_quant"}[case["what"]]
    return stem + ("_h<" if case["dtype"] == "f16" else "<")


def gmm_check(case, got, ref, what):
    """mean and variance: test_gpu_gmm.check (its TOL); the queries: bit identity"""
    if case["what"] in ("mean", "variance"):
        test_gpu_gmm.check(got, ref, what)
    else:
        test_gpu_gmm_f16.check(got, ref, what)


@pytest.mark.parametrize("seed", range(rc.SWEEPS["gmm"][1]))
def test_random_gmm_query_case(pkg, orc, gpu, tune, seed):
    import torch
    t0 = time.perf_counter()
    case = rc.gmm_case(seed)
    what = f"seed {seed}: {case}"
    m = camera(pkg, case)
    set_knobs(tune, case)
    upload, wide = gmm_records(orc, case)
    pkg.init_gmm(*upload)
    assert pkg.gmm_dtype() == case["dtype"], what
    set_gmm_query(pkg, case)
    if case["baked"]:
        {"mean": pkg.bake_gmm_stats, "variance": pkg.bake_gmm_stats, "range": pkg.bake_gmm_range,
         "crossing": pkg.bake_gmm_range, "quantile": pkg.bake_gmm_quantile}[case["what"]]()
        got = render_frame(pkg, torch, case, m, pkg.render_gmm_baked, volume_size=(1, 1, 1))
        kernel = pkg.last_kernel()
        if case["what"] == "crossing":
            assert kernel == PLANE_KERNEL, f"{what}: {kernel}"
        else:
            assert "<B=1,M=0>" in kernel and not kernel.startswith("k_march_gmm"), \
                f"{what}: {kernel}"
    else:
        got = render_frame(pkg, torch, case, m, pkg.render_gmm, volume_size=(1, 1, 1))
        kernel = pkg.last_kernel()
        assert kernel.startswith(gmm_march_name(case)) and \
            f"<B={case['K']},M={case['method']}>" in kernel, f"{what}: {kernel}"
    gmm_check(case, got, gmm_reference(pkg, orc, case, wide, m), f"{what} kernel {kernel}")
    report(case, kernel, t0)


@pytest.mark.parametrize("seed", range(rc.SWEEPS["chain"][1]))
def test_random_gmm_chain_case(pkg, orc, gpu, tune, seed):
    """a chain of 2-4 z-slabs, each resident alone with its halo slice, the alive list
    handed on: the final frame is the whole-volume reference frame, and for the
    mean and the variance, which the oracle marches slab by slab too, every
    hand-off's alive count and ray entries are the oracle's.  With the eye inside
    the volume the slabs in front of it take no sample and hand every ray on."""
    import torch
    t0 = time.perf_counter()
    case = make_case(pkg, "chain", seed)
    what = f"seed {seed}: {case}"
    W, H, dims = case["W"], case["H"], case["dims"]
    m = camera(pkg, case)
    direction = pkg.slabs.march_direction(m, W, H)
    assert direction != 0, what
    bounds = pkg.slabs.slab_bounds(dims[2], case["nslabs"], direction)
    set_knobs(tune, case)
    upload, wide = gmm_records(orc, case)
    set_gmm_query(pkg, case)
    out = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    out_f = torch.zeros(H * W * 4, dtype=torch.float32, device="cuda")
    steps = torch.full((H * W,), -2, dtype=torch.int32, device="cuda")
    d = pkg.make_desc(out, W, H, m, d_output_f=out_f, d_steps=steps, volume_size=(1, 1, 1),
                      **desc_kw(case))
    bufs = [torch.zeros((W * H, pkg.slabs.RAY_WORDS), dtype=torch.int32, device="cuda")
            for _ in range(2)]
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    oracle_chain = case["what"] in ("mean", "variance")
    p = oracle_params(orc, case, m)
    pix = lambda a: a[:, 8] & 0x7FFFFF  # the entry's last word: pixel | samples << 23
    n_in, ref_rays, carried, kernels = 0, None, [], set()
    for i, (z_lo, z_hi) in enumerate(bounds):
        zb, ns = pkg.slabs.resident_slices(z_lo, z_hi, dims[2])
        pkg.init_gmm(upload[0][zb:zb + ns], upload[1][zb:zb + ns], dims, z_base=zb)
        rin = bufs[(i + 1) % 2] if i else None
        s = pkg.gmm_slab(z_lo, z_hi, bufs[i % 2], cnt[0:1], d_rays_in=rin, n_rays_in=n_in)
        pkg.render_gmm(d, s)
        torch.cuda.synchronize()
        kernels.add(pkg.last_kernel())
        assert pkg.last_kernel().startswith(gmm_march_name(case)), f"{what}: {pkg.last_kernel()}"
        n_in = int(cnt[0].item())
        carried.append(n_in)
        if oracle_chain:
            r = orc.render_gmm(wide[0][zb:zb + ns], wide[1][zb:zb + ns], dims, p, z_base=zb,
                               slab=(z_lo, z_hi), rays_in=ref_rays)
            ref_rays = r["rays_out"]
            assert n_in == ref_rays.shape[0], \
                f"{what}: slab {i}: {n_in} alive rays vs {ref_rays.shape[0]}"
            got_rays = bufs[i % 2][:n_in].cpu().numpy().view(np.uint32)
            assert np.array_equal(got_rays[np.argsort(pix(got_rays), kind="stable")],
                                  ref_rays[np.argsort(pix(ref_rays), kind="stable")]), \
                f"{what}: slab {i}: alive-list entries differ"
    assert n_in == 0, f"{what}: rays alive after the last slab: {carried}"
    got = (out.cpu().numpy().view(np.uint32).reshape(H, W), out_f.cpu().numpy().reshape(H, W, 4),
           steps.cpu().numpy().reshape(H, W))
    gmm_check(case, got, gmm_reference(pkg, orc, case, wide, m),
              f"{what} carried {carried} {sorted(kernels)}")
    report(case, kernels, t0)
