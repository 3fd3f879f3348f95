"""Seeded random parity sweep of the lit march: what test_gpu_random_transfer.py does
for the table marches, for

  k_march_lit (headlight gradient shading of a frame from a baked plane,
  vr_shade.hip): whole frames and multi-rank tile lists
  assembled by k_unscatter, from the baked planes of record volumes (fp32 and f16;
  methods 1/2/3 and 10-13), codec volumes (4/5/6), their gradient-magnitude planes
  (32 + method, section 26) and GMM volumes (1, 2, 10, 11, 13 through render_gmm_baked).

Every case is random_cases' dict of its seed (lit_case, lit_tile_case): tf_case's
deals -- an nx around the planes' 15-voxel brick pitch with two, three or five rows, the
camera inside the volume or along an axis, frames from 1 x 1, every table size and
kind, negated windows, VR_TF_WIDE -- and besides the plane (the method's or its
gradient plane), no table at all (the built-in nine entries) and the light (ambient,
diffuse, specular, shininess 2^0 .. 2^7; the identity twice; coefficients that saturate).
Every comparison is exact: packed RGBA8, float RGBA and samples per pixel are
np.array_equal to tests/ref_shading.py marching the plane numpy computes per voxel
(test_random_cases.tf_plane), for a gradient case ref_gradient.gradient_plane of that
plane.  One exception, test_gpu_random_transfer.py's: a GMM volume's mean and variance
planes have no bit-exact numpy restatement, so for those two the reference marches the
plane the device holds.

A whole frame is rendered three times from one descriptor and compared each time (the
estimate tile order, the order re-dealt by the recorded costs, the steady order); under
the identity light it must also be the unlit k_march_plane_tf frame.
tests/test_random_planes.py checks on the CPU that the reference frames are worth
comparing and that the sweep would notice an ignored light, an unscaled gradient, a
shininess off by one, exchanged coefficients, a lit alpha or a gradient plane replaced
by its source.  A failure message carries the seed and the whole case.

Seconds per case on one MI355X, reference included (the CASE lines of a run with -s):
lit 0.05 mean / 0.16 at most, tile lists 0.09 / 0.21; the 56 cases take 5 s.
"""
import time

import numpy as np
import pytest

import random_cases as rc
from test_gpu_random_queries import assert_same, render_frame, report, set_knobs
from test_gpu_random_transfer import TF_BLEND, TF_CROSS, bake_planes, frame_call
from test_random_cases import camera
from test_random_planes import lit_reference, with_gradients

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    """no light, no table, no query state, no planes, no tuning knob, the default stream
    and no volume of any kind, before and after"""
    def drop():
        pkg.set_light(None)
        pkg.set_transfer_function(None)
        pkg.set_transfer_function_2d(None)
        pkg.clear_tuning()
        pkg.set_stream(None)
        pkg.set_crossing_weights(None)
        pkg.set_query_target(None)
        pkg.set_quantile(None)
        pkg.set_bin_weights(None)
        pkg.release_stats()
        pkg.clear_gmm_range()
        pkg.release_gmm_stats()
        pkg.release_gmm_range()
        pkg.release_gmm_quantile()
        for slot in (1, 0):
            pkg.gmm_select(slot)
            pkg.free_gmm()
        pkg.freeCudaBuffers()
    drop()
    yield
    drop()


def kernel_name(case):
    """a gradient plane is blended, never combined"""
    return f"k_march_lit<B=1,M={13 if case['plane'] == 13 else 0}>"


def bake_lit_planes(pkg, orc, case, what):
    """test_gpu_random_transfer.bake_planes and, for a gradient case, the gradient plane
    of the method; returns {the case's plane: what the reference marches}"""
    sources = bake_planes(pkg, orc, case, what)
    if case["grad"]:
        pkg.bake_gradient(case["u"])
        assert pkg.last_kernel().startswith("k_bake_grad"), what
    return with_gradients(case, sources)


def set_table_and_light(pkg, case):
    pkg.set_transfer_function(None if case["table"] is None else rc.make_table(case["table"]))
    ka, kd, ks, k = case["light"]
    pkg.set_light(ka, kd, ks, 1 << k)


@pytest.mark.parametrize("seed", range(rc.PLANE_SWEEPS["lit"][1]))
def test_random_lit_case(pkg, orc, gpu, tune, seed):
    """a whole lit frame, three times"""
    import torch
    t0 = time.perf_counter()
    case = rc.lit_case(seed)
    what = f"seed {seed}: {case}"
    m = camera(pkg, case)
    planes = bake_lit_planes(pkg, orc, case, what)
    set_table_and_light(pkg, case)
    set_knobs(tune, case)
    ref = lit_reference(case, planes, m)
    call, kw = frame_call(pkg, case)
    frame = dict(case, method=case["plane"])
    resident = pkg.layout_info()["resident_bytes"]
    for order in ("estimate order", "re-dealt order", "steady order"):
        got = render_frame(pkg, torch, frame, m, call, **kw)
        kernel = pkg.last_kernel()
        assert kernel == kernel_name(case), f"{what}: {order}: {kernel}"
        assert_same(got, ref, f"{what} kernel {kernel}, {order}")
    if case["light"] == rc.IDENTITY_LIGHT:  # the unlit frame of the table march
        assert case["table"] is not None, what
        pkg.set_light(None)
        unlit = render_frame(pkg, torch, frame, m, call, **kw)
        assert pkg.last_kernel() == (TF_CROSS if case["plane"] == 13 else TF_BLEND), \
            f"{what}: {pkg.last_kernel()}"
        assert_same(unlit, ref, f"{what}: the unlit frame")
    assert pkg.layout_info()["resident_bytes"] == resident, what  # no layout copy made
    report(case, kernel, t0)


@pytest.mark.parametrize("seed", range(rc.PLANE_SWEEPS["littiles"][1]))
def test_random_lit_tile_list_case(pkg, orc, gpu, tune, seed):
    """a multi-GPU split of a lit frame: every rank's tile list rendered into
    sentinel-filled packed slots, the slots assembled by k_unscatter, equals the
    reference frame"""
    import torch
    t0 = time.perf_counter()
    case = rc.lit_tile_case(seed)
    what = f"seed {seed}: {case}"
    W, H, world = case["W"], case["H"], case["world"]
    m = camera(pkg, case)
    planes = bake_lit_planes(pkg, orc, case, what)
    set_table_and_light(pkg, case)
    set_knobs(tune, case)
    call, kw = frame_call(pkg, case)
    p = case["params"]
    lists = pkg.tiles.tile_lists(W, H, world, m)
    n_slots = lists.shape[1]
    packed = torch.full((world, n_slots * 256), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dl = torch.from_numpy(lists.view(np.int32).copy()).cuda()
    for r in range(world):
        call(pkg.make_desc(packed[r], W, H, m, d_tile_list=dl[r], n_tiles=n_slots,
                           density=p["density"], brightness=p["brightness"],
                           transfer_offset=p["toff"], transfer_scale=p["tscale"],
                           query_method=case["plane"], **kw))
        assert pkg.last_kernel() == kernel_name(case), f"{what}: rank {r}: {pkg.last_kernel()}"
    frame = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    pkg.unscatter_tiles(packed, dl, world, n_slots, frame, W, H)
    torch.cuda.synchronize()
    got = frame.cpu().numpy().view(np.uint32).reshape(H, W)
    ref = lit_reference(case, planes, m)[0]
    assert np.array_equal(got, ref), \
        f"{what} {kernel_name(case)}: {int(np.sum(got != ref))} pixels differ"
    report(case, kernel_name(case), t0)
