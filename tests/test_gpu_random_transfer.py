"""Seeded random parity sweep of the two table marches: what test_gpu_random.py and
test_gpu_random_queries.py do for the other marches, for

  k_march_plane_tf (a 1-D user transfer function, vr_transfer.hip, DESIGN.md
  section 22) and k_march_tf2 (a 2-D table over two planes, vr_transfer2.hip,
  section 23): whole frames and multi-rank tile lists assembled by k_unscatter, from
  the baked planes of record volumes (fp32 and f16; methods 1/2/3 and 10-13), codec
  volumes (4/5/6) and GMM volumes (1, 2, 10, 11, 13 through render_gmm_baked).

Every case is random_cases' dict of its seed (tf_case, tf2_case, tf_tile_case): the
volume may have an nx around the planes' 15-voxel brick pitch and two, three or five
rows, the camera may sit inside it or look along an axis, the frame is anything from
1 x 1, the table has any of the sizes the staging loops treat differently and
entries in [0, 1), of 8 bits, or outside [0, 1] (an alpha above 1 or below 0 is
legal), the windows may be negated, and VR_TF_WIDE picks the 64-bit plane indices.
Every comparison is exact: packed RGBA8, float RGBA and samples per pixel are
np.array_equal to tests/ref_transfer.py or tests/ref_transfer2.py marching the planes
numpy computes per voxel (test_random_cases.tf_plane).  One exception, in the
planes and not in the march: a GMM volume's mean and variance planes meet the
oracle within 1e-4 and have no bit-exact numpy restatement (tests/test_gpu_gmm_baked.py
holds them), so for those two the reference marches the plane the device holds, read
back as test_gpu_transfer2._gmm_plane reads it.

A whole frame is rendered three times from one descriptor and compared each time:
the first frame of a view runs in the estimate tile order and records tile costs,
the second in the order re-dealt by them, the third in the steady one (frame_order
in vr_api.cpp, record_tile_cost at the end of both kernels).
tests/test_random_cases.py checks on the CPU that the reference frames are worth
comparing and that the sweep would notice an ignored axis, exchanged blends or
planes, or a wrong window.  A failure message carries the seed and the whole case.

Seconds per case on one MI355X, reference included (the CASE lines of a run with
-s): tf 0.04 mean / 0.16 at most, tf2 0.05 / 0.16, tile lists 0.08 / 0.29; the 144
cases take 10 s.
"""
import math
import time

import numpy as np
import pytest

import random_cases as rc
from test_gpu_random_queries import (assert_same, bake_query, render_frame, report, set_knobs,
                                     set_query)
from test_gpu_transfer2 import _gmm_plane, kernel_of
from test_random_cases import (axis_case, camera, tf_methods, tf_plane, tf_records, tf_reference)

pytestmark = pytest.mark.gpu

TF_BLEND = "k_march_plane_tf<B=1,M=0>"
TF_CROSS = "k_march_plane_tf<B=1,M=13>"


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    """no table, no query state, no planes, no tuning knob, the default stream and no
    volume of any kind, before and after"""
    def drop():
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
    if case["v"] is None:
        return TF_CROSS if case["u"] == 13 else TF_BLEND
    return kernel_of(case["u"], case["v"])


def bake_planes(pkg, orc, case, what):
    """upload the family's records, set the query state of the case's methods, bake
    exactly the planes they read; returns {method: the plane the reference marches}"""
    methods = tuple(dict.fromkeys(tf_methods(case)))
    records = tf_records(orc, case)
    if case["family"] == "records":
        pkg.init_distribution(records)
        assert pkg.volume_dtype() == case["dtype"], what
        for mth in methods:
            if mth >= 10:
                set_query(pkg, axis_case(case, mth))
        if any(mth <= 3 for mth in methods):
            pkg.bake_stats()
        for mth in methods:
            if mth >= 10:
                bake_query(pkg, mth)
    elif case["family"] == "codec":
        pkg.init_codec(*records)
        pkg.bake_stats()
    else:
        pkg.init_gmm(*records[0])
        assert pkg.gmm_dtype() == case["dtype"], what
        q = case["queries"]
        if 13 in methods:
            pkg.set_gmm_range(-math.inf, q[13]["theta"])
        elif 10 in methods:
            pkg.set_gmm_range(q[10]["lo"], q[10]["hi"])
        if 11 in methods:
            if q[11]["state"] == "spread":
                pkg.set_quantile_spread(q[11]["lo"], q[11]["hi"])
            else:
                pkg.set_quantile(q[11]["q"])
        if 1 in methods or 2 in methods:
            pkg.bake_gmm_stats()
        if 10 in methods or 13 in methods:
            pkg.bake_gmm_range()
        if 11 in methods:
            pkg.bake_gmm_quantile()
        pkg.free_gmm()  # the planes need no records
    planes = {}
    for mth in methods:
        if case["family"] == "gmm" and mth <= 2:
            # no bit-exact restatement of these two planes (module docstring): the
            # device's own, whose values are tests/test_gpu_gmm_baked.py's business
            planes[mth] = _gmm_plane(pkg.gmm_stats_info(), mth - 1)
        else:
            planes[mth] = tf_plane(pkg, orc, case, mth, records)
        assert planes[mth].shape == case["dims"][::-1], what
    return planes


def set_table(pkg, case):
    table = rc.make_table(case["table"])
    if case["v"] is None:
        pkg.set_transfer_function(table)
    else:
        pkg.set_transfer_function_2d(table, case["v"], case["voff"], case["vscale"])


def frame_call(pkg, case):
    """(the render entry point of the case's family, its extra descriptor fields)"""
    if case["family"] == "gmm":
        return pkg.render_gmm_baked, dict(volume_size=(1, 1, 1))
    return pkg.render, {}


def whole_frame_case(pkg, orc, tune, case):
    import torch
    t0 = time.perf_counter()
    what = f"seed {case['seed']}: {case}"
    m = camera(pkg, case)
    planes = bake_planes(pkg, orc, case, what)
    set_table(pkg, case)
    set_knobs(tune, case)
    ref = tf_reference(case, planes, m)
    call, kw = frame_call(pkg, case)
    resident = pkg.layout_info()["resident_bytes"]
    # one descriptor three times: the estimate tile order with the costs recorded,
    # the order re-dealt by them, the steady order
    for order in ("estimate order", "re-dealt order", "steady order"):
        got = render_frame(pkg, torch, dict(case, method=case["u"]), m, call, **kw)
        kernel = pkg.last_kernel()
        assert kernel == kernel_name(case), f"{what}: {order}: {kernel}"
        assert_same(got, ref, f"{what} kernel {kernel}, {order}")
    assert pkg.layout_info()["resident_bytes"] == resident, what  # no layout copy made
    report(case, kernel, t0)


@pytest.mark.parametrize("seed", range(rc.SWEEPS["tf"][1]))
def test_random_transfer_case(pkg, orc, gpu, tune, seed):
    """a whole frame under a 1-D table, three times"""
    whole_frame_case(pkg, orc, tune, rc.tf_case(seed))


@pytest.mark.parametrize("seed", range(rc.SWEEPS["tf2"][1]))
def test_random_transfer2_case(pkg, orc, gpu, tune, seed):
    """a whole frame under a 2-D table over two planes, three times"""
    whole_frame_case(pkg, orc, tune, rc.tf2_case(seed))


@pytest.mark.parametrize("seed", range(rc.SWEEPS["tftiles"][1]))
def test_random_transfer_tile_list_case(pkg, orc, gpu, tune, seed):
    """a multi-GPU split of a frame under a table: every rank's tile list rendered
    from the planes into sentinel-filled packed slots, the slots assembled by
    k_unscatter, equals the reference frame -- the route bench.py --gpus N would take
    with a table set"""
    import torch
    t0 = time.perf_counter()
    case = rc.tf_tile_case(seed)
    what = f"seed {seed}: {case}"
    W, H, world = case["W"], case["H"], case["world"]
    m = camera(pkg, case)
    planes = bake_planes(pkg, orc, case, what)
    set_table(pkg, case)
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
                           query_method=case["u"], **kw))
        assert pkg.last_kernel() == kernel_name(case), f"{what}: rank {r}: {pkg.last_kernel()}"
    frame = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    pkg.unscatter_tiles(packed, dl, world, n_slots, frame, W, H)
    torch.cuda.synchronize()
    got = frame.cpu().numpy().view(np.uint32).reshape(H, W)
    ref = tf_reference(case, planes, m)[0]
    assert np.array_equal(got, ref), \
        f"{what} {kernel_name(case)}: {int(np.sum(got != ref))} pixels differ"
    report(case, kernel_name(case), t0)
